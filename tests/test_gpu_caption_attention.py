"""The caption's two softmax attentions on exact and adversarial inputs (tests/caption_attention_cases.py; its preconditions and
the proof that these assertions reject a subtly wrong kernel are in tests/test_caption_attention_cases.py): the decode step
(ops.llama_decode_attention, decode_rows.llama_decode_attention_rows: da_kernel + da_combine_kernel) and the flash prefill
(prefill_attention.llama_prefill_attention), fp16 and bf16, at every group size 1 .. 8, at caches shorter than one key chunk and
at 66 chunks, where da_combine_kernel takes its second round.

  needle    ``torch.equal`` with the target key's V row: no tolerance
  counting  |got - c_d / (p + 1)| <= one spacing of T, and round(got (p + 1)) == c_d: every key up to the position counted once
  ramp      per row max_d |got - want| <= tol_T max_d |want_row| against an fp64 softmax, tol_T = 4e-3 / 3e-2

After every decode call the cache differs from its copy at slot ``pos`` only and holds the expected new key and value there.

Measured maxima of error / bound (MI355X, every case below; fp16 / bf16), the needle being equal everywhere:
    decode step   counting 0.37 / 0.30   ramp 0.11 / 0.13
    prefill       counting 0.50 / 0.50   ramp 0.14 / 0.18
(0.50 of a spacing is the one rounding to T.)  No case failed when these tests were first run: no fault was found in either kernel."""
import pytest
import torch

import caption_attention_cases as CA
from test_gpu_prefill_attention import HD, TOL, _inputs, _reference

pytestmark = pytest.mark.gpu

_DT = pytest.mark.parametrize("dtype", CA.DTYPES, ids=CA.DTN.get)
_PID = lambda s: "t%d_p%d_q%d_kv%d_m%d" % s


def _prefill(cuda, c):
    from rsvld_amd import prefill_attention as PA
    return PA.llama_prefill_attention(c.q.to(cuda), c.k.to(cuda), c.v.to(cuda), c.n_q, c.n_kv, CA.SCALE, pos0=c.pos0)


def _check_cache(c, kc, vc, k0, v0):
    """The call wrote slot ``pos`` of both caches, the expected rows, and nothing else."""
    for cache, orig, new in ((kc, k0, c.new_k), (vc, v0, c.new_v)):
        changed = (cache != orig).any(dim=-1).any(dim=0).nonzero().flatten().tolist()
        assert changed == [c.pos], f"{c.label}: the call changed cache slots {changed[:8]}"
        assert torch.equal(cache[:, c.pos].cpu(), new), f"{c.label}: slot {c.pos} does not hold the new row"


def _decode(cuda, c):
    from rsvld_amd import ops
    kc, vc = c.kc.to(cuda), c.vc.to(cuda)
    k0, v0 = kc.clone(), vc.clone()
    got = ops.llama_decode_attention(c.qkv.to(cuda), c.cos.to(cuda), c.sin.to(cuda), torch.tensor([c.pos], device=cuda), kc, vc,
                                     c.n_q, c.n_kv, CA.SCALE)
    assert got.shape == (c.n_q * HD,) and got.dtype == c.dtype
    _check_cache(c, kc, vc, k0, v0)
    return got


def _walk(cases, run):
    """Run and check every case; -> {family: worst error / bound}.  Every case is run before the first failure is raised."""
    worst, failures = {}, []
    for c in cases:
        try:
            r = CA.check(c, run(c))
        except AssertionError as e:
            failures.append(str(e))
            continue
        print(f"{c.label} {CA.DTN[c.dtype]}: worst error / bound = {r:.3g}")
        worst[c.family] = max(worst.get(c.family, 0.0), r)
    assert not failures, "\n".join(failures)
    return worst


@_DT
@pytest.mark.parametrize("shape", CA.PREFILL_BASE + CA.PREFILL_GROUPS, ids=_PID)
def test_prefill_on_needle_counting_and_ramp(cuda, shape, dtype):
    """All T rows of a call against all keys at once; g = 2 .. 7 beside the suite's 4: one token's heads straddle waves and workgroups."""
    print(_walk(CA.prefill_cases(dtype, [shape]), lambda c: _prefill(cuda, c)))


@_DT
@pytest.mark.parametrize("case", CA.PREFILL_GROUPS, ids=_PID)
def test_prefill_group_sizes_against_cpu_fp32_reference(cuda, case, dtype):
    """The assertion of test_gpu_prefill_attention.test_kernel_against_cpu_fp32_reference, on the group sizes it does not launch."""
    from rsvld_amd import prefill_attention as PA
    T, pos0, n_q, n_kv, max_len = case
    q, k, v = _inputs(*case, dtype)
    got = PA.llama_prefill_attention(q.to(cuda), k.to(cuda), v.to(cuda), n_q, n_kv, HD ** -0.5, pos0=pos0)
    assert got.shape == (T, n_q * HD) and got.dtype == dtype and got.is_contiguous()
    want = _reference(*case, dtype)
    err = float((got.float().cpu() - want).abs().max())
    bound = TOL[dtype] * float(want.abs().max()) + 1e-6
    print(f"prefill attention {case} {dtype}: max|d| = {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound, (err, bound)


@_DT
@pytest.mark.parametrize("group", CA.DECODE_GROUPS, ids=lambda g: "q%d_kv%d" % g)
def test_decode_step_on_needle_counting_and_ramp(cuda, group, dtype):
    """G = 1 .. 8 query heads per kv head; one key, both sides of the 128-key chunk boundary, mid-chunk, the last slot, and a cache
    shorter than one chunk."""
    cases = CA.decode_cases(*group, CA.DECODE_POSITIONS, dtype, group in CA.DECODE_RAMP_GROUPS)
    print(_walk(cases, lambda c: _decode(cuda, c)))


@_DT
def test_decode_combine_second_round(cuda, dtype):
    """66 key chunks: da_combine_kernel folds 64, then 2, and brings both rounds to the larger maximum.  Round two empty (100), round one
    just full (8191), one key in round two (8192), the last slot (8324); the needle's targets lie in the other round from the row,
    the ramp's a = +-4 heads rescale in both directions."""
    print(_walk(CA.combine_cases(dtype), lambda c: _decode(cuda, c)))


@_DT
def test_decode_combine_second_round_rows_equal_single_calls(cuda, dtype):
    """The same through llama_decode_attention_rows, B = 3 at positions (100, 8192, 8324): bit-identical to three single calls, and
    every row passes its family's assertion."""
    from rsvld_amd import decode_rows as DR
    n_q, n_kv = CA.COMBINE_GROUP
    by_family = {}
    for c in CA.combine_cases(dtype, CA.COMBINE_ROWS):
        by_family.setdefault(c.label.split()[-1], []).append(c)
    assert sorted(by_family) == ["counting", "needle", "ramp/saw", "ramp/up"]
    for name, cs in by_family.items():
        assert [c.pos for c in cs] == CA.COMBINE_ROWS
        want = torch.stack([_decode(cuda, c) for c in cs])
        kb, vb = torch.stack([c.kc for c in cs]).to(cuda), torch.stack([c.vc for c in cs]).to(cuda)
        k0, v0 = kb.clone(), vb.clone()
        got = DR.llama_decode_attention_rows(torch.stack([c.qkv for c in cs]).to(cuda), torch.stack([c.cos for c in cs]).to(cuda),
                                             torch.stack([c.sin for c in cs]).to(cuda), torch.tensor(CA.COMBINE_ROWS, device=cuda), kb, vb,
                                             n_q, n_kv, CA.SCALE)
        assert torch.equal(got, want), name
        for b, c in enumerate(cs):
            _check_cache(c, kb[b], vb[b], k0[b], v0[b])
            CA.check(c, got[b])
