"""The cases of tests/test_gpu_caption_attention.py, walked on the CPU (tests/caption_attention_cases.py): the builders'
preconditions are PROVEN here, none is assumed; the fp64 reference rounded once to T passes every assertion on every case (the
cases are fair); and every fault of ``FAULTS`` built into that reference is rejected by at least one of them (they have teeth)."""
import pytest
import torch

import caption_attention_cases as CA

F16, BF16 = CA.F16, CA.BF16
_DT = pytest.mark.parametrize("dtype", CA.DTYPES, ids=CA.DTN.get)
BASE300 = CA.PREFILL_BASE[0]


def _needles(dtype):
    return [c for c in CA.all_cases(dtype) if c.family == "needle"]


def test_the_tables_name_the_shapes_the_kernels_branch_on():
    groups = sorted({n_q // n_kv for _, _, n_q, n_kv, _ in CA.PREFILL_BASE + CA.PREFILL_GROUPS})
    assert groups == [2, 3, 4, 5, 6, 7] and all(128 % g and 32 % g for g in (3, 5, 6, 7))
    assert sorted({n_q // n_kv for n_q, n_kv in CA.DECODE_GROUPS}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert all(pos < max_len for max_len, pos in CA.DECODE_POSITIONS) and (100, 99) in CA.DECODE_POSITIONS      # a cache shorter than one chunk
    chunks = (CA.COMBINE_MAX_LEN + 127) // 128
    assert chunks == 66 and 64 * 128 == 8192 and set(CA.COMBINE_ROWS) <= set(CA.COMBINE_POSITIONS)


def test_the_seventh_family_is_p_minus_25():
    """Why the "scatter" variant exists: (37 p + 11) mod (p + 1) = p - 25 from p = 26 on, no pseudo-random key."""
    assert all(CA.needle_target(p, 6, 0) == p - 25 for p in range(26, 9000))


@_DT
def test_needle_leak_is_below_2_pow_minus_12_in_every_row(dtype):
    worst = 0.0
    for c in _needles(dtype):
        leak = CA.needle_leak(c)
        assert float(leak.max()) < CA.LEAK_BOUND, (c.label, float(leak.max()))
        assert int(c.targets.min()) >= 0 and bool((c.targets <= torch.tensor(c.positions)[:, None]).all()), c.label
        worst = max(worst, float(leak.max()))
    print(f"needle, {CA.DTN[dtype]}: worst leak {worst:.3e} (bound {CA.LEAK_BOUND:.3e})")


def test_every_needle_family_occurs_for_every_group_size():
    for shape in CA.PREFILL_BASE + CA.PREFILL_GROUPS:
        T, pos0, n_q, n_kv, _ = shape
        assert {(t + h) % 8 for t in range(T) for h in range(n_q)} == set(range(8)), shape
    for n_q, n_kv in CA.DECODE_GROUPS:
        assert {(t + h) % 8 for t in range(len(CA.DECODE_POSITIONS)) for h in range(n_q)} == set(range(8)), (n_q, n_kv)
    c = CA.needle_decode(8, 2, 384, 300, 3, BF16)                    # the targets are what the table says
    assert c.targets.tolist() == [[CA.needle_target(300, 3, h) for h in range(8)]]
    assert sorted(c.targets[0].tolist()) == sorted([300, 0, 299, 256, 255, 255, 275, 63])


def test_every_key_of_the_300_token_call_is_a_target():
    """With 8 query heads every token has a row of every family, the first of which is its own key.  (A call with fewer heads, or
    one that starts above position 0, has fewer rows of that family than keys: there it is the counting family that says every
    key was read.)"""
    c = CA.needle_prefill(BASE300, BF16)
    assert sorted(set(c.targets.flatten().tolist())) == list(range(300))


def test_every_in_tile_offset_is_a_target_below_the_rows_own_tile():
    """Over the rows of the 300-token call: the table alone reaches offsets 0 and 39 .. 63 in a tile strictly below the row's own
    (see test_the_seventh_family_is_p_minus_25), the scatter variant all 64."""
    def below(c):
        p = torch.tensor(c.positions)[:, None].expand_as(c.targets)
        return set((c.targets[c.targets // 64 < p // 64] % 64).tolist())
    assert below(CA.needle_prefill(BASE300, BF16, "table")) == {0} | set(range(39, 64))
    assert below(CA.needle_prefill(BASE300, BF16, "scatter")) == set(range(64))


@_DT
def test_decode_cases_hand_the_kernel_the_pre_image_of_the_rotation(dtype):
    for c in CA.decode_cases(8, 2, CA.DECODE_POSITIONS, dtype, True):
        qkv = c.qkv.double().reshape(c.n_q + 2 * c.n_kv, CA.HD)
        assert set(c.cos.unique().tolist()) <= {0.0, 1.0, -1.0} and bool(((c.cos == 0) != (c.sin == 0)).all())
        assert torch.equal(c.cos[:64], c.cos[64:]) and torch.equal(c.sin[:64], c.sin[64:])
        rot = CA.rope(qkv[:c.n_q + c.n_kv], c.cos.double(), c.sin.double())
        assert torch.equal(rot[:c.n_q], c.q64[0]) and torch.equal(rot[c.n_q:], c.k64[:, c.pos]), c.label
        assert torch.equal(qkv[c.n_q + c.n_kv:], c.v64[:, c.pos])
        # the stale row differs from what the call writes, and the slots above hold the decoys
        assert not torch.equal(c.kc[:, c.pos], c.new_k) and not torch.equal(c.vc[:, c.pos], c.new_v)
        assert bool((c.vc[:, c.pos + 1:] == 100).all())
        assert torch.equal(c.kc[:, :c.pos].double(), c.k64[:, :c.pos]) and torch.equal(c.vc[:, :c.pos].double(), c.v64[:, :c.pos])


@_DT
def test_the_rounded_fp64_reference_passes_every_case(dtype):
    worst = {}
    for c in CA.all_cases(dtype):
        r = CA.check(c, CA.reference(c))
        worst[c.family] = max(worst.get(c.family, 0.0), r)
    print(f"ideal kernel, {CA.DTN[dtype]}: worst ratio to the bound {worst}")
    assert worst["needle"] == 0.0 and worst["counting"] <= 0.5 and worst["ramp"] <= 0.5


def _rejects(c, fault):
    try:
        CA.check(c, CA.reference(c, fault=fault))
    except AssertionError:
        return True
    return False


@_DT
@pytest.mark.parametrize("fault", sorted(CA.FAULTS), ids=lambda f: f"fault{f}")
def test_every_fault_is_rejected(fault, dtype):
    caught = next((c for c in CA.all_cases(dtype) if _rejects(c, fault)), None)
    assert caught is not None, f"no case rejects: {CA.FAULTS[fault]}"
    print(f"fault {fault} ({CA.FAULTS[fault]}): rejected by {caught.label}")


@_DT
def test_faults_are_rejected_where_the_families_are_meant_to_see_them(dtype):
    """Single-key faults at the lengths where a whole-output tolerance lets them pass: the needle and the counting family reject
    them at 8 325 keys as at 100."""
    last = {c.label.split()[-1]: c for c in CA.combine_cases(dtype, [8324])}
    for fault in (1, 2, 4):
        assert _rejects(last["counting"], fault), fault
    # a whole chunk dropped leaves the counts uniform (64 / 8197 = 65 / 8325 to 1e-5): at 8324 it is the rising ramp that sits on the
    # last chunks, and at 8192 the one key of round two is the needle's target and a count of its own
    assert _rejects(last["ramp/up"], 7) and _rejects(last["ramp/up"], 6)
    one = {c.label.split()[-1]: c for c in CA.combine_cases(dtype, [8192])}
    assert _rejects(one["counting"], 7) and _rejects(one["needle"], 7)
    stale = [c for c in CA.decode_cases(8, 2, CA.DECODE_POSITIONS, dtype, False) if c.family == "needle" and c.pos in c.targets[0].tolist() and c.pos > 0]
    assert stale and all(_rejects(c, 3) for c in stale)
    p300 = CA.needle_prefill(BASE300, dtype)
    assert all(_rejects(p300, f) for f in (1, 2, 5, 6))
    assert _rejects(CA.ramp_prefill(BASE300, dtype, "up"), 8) and _rejects(CA.counting_prefill(BASE300, dtype), 4)
