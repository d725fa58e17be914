"""The public switches of the MFMA decode attention, walked on the CPU: CaptionMode.decode_attention, caption_mode's fourth value,
PipelineConfig.caption_attention, --caption_attention on both command lines, the host-only plan (rsvld_plan_llama_decode_attention_mma)
and the workspace size on the built library.  And the cases tests/test_gpu_caption_decode_attention_mma.py runs at ITS positions -- both
sides of every 32-key wave block, 64-key tile and range boundary -- walked as tests/test_caption_attention_cases.py walks the suite's:
the rounded fp64 reference passes every one, and every fault that can occur at those boundaries is rejected by at least one.  Three
faults the evaluator of caption_attention_cases cannot express are built here around ``CA.reference``: the last key of a range dropped,
one wave's partial dropped in the merge inside a workgroup, the rotated q of another sequence.  The kernels themselves:
tests/test_gpu_caption_decode_attention_mma.py, tests/test_gpu_caption_decode_attention_mode.py."""
import types

import pytest
import torch

import caption_attention_cases as CA

_DT = pytest.mark.parametrize("dtype", CA.DTYPES, ids=CA.DTN.get)


def plan(n_q, n_kv, max_len, dtype=None):
    from rsvld_amd import decode_rows as DR
    return DR.plan_decode_attention_mma(n_q, n_kv, max_len, dtype)


def range_keys():
    return int(plan(8, 2, 384).range_keys)


def positions(R):
    """(max_len, pos) of the exact families: the 32-key wave blocks and the 64-key tile of range 0, both sides of the first two range
    boundaries, the last slot, and caches shorter than one range and than one tile."""
    return ([(384, p) for p in (0, 31, 32, 63, 64, 65)] + [(384, p) for p in (R - 1, R, R + 1, 2 * R - 1, 2 * R)]
            + [(384, 383), (100, 99), (40, 39)])


def combine_shape(R):
    """66 ranges -> (max_len, positions): round two of the combine empty, round one just full, one key in round two, the last slot."""
    max_len = 65 * R + 5
    return max_len, [100, 64 * R - 1, 64 * R, max_len - 1]


# ---- the switches
def test_caption_mode_has_a_sixth_field_last():
    import dataclasses
    from rsvld_amd import llava_next as LN, ops
    assert LN.CAPTION_ATTENTIONS == ("valu", "mfma") == ops.DECODE_ATTENTION_KERNELS
    assert [f.name for f in dataclasses.fields(LN.CaptionMode)][-1] == "decode_attention" and len(dataclasses.fields(LN.CaptionMode)) == 6
    assert LN.CaptionMode().decode_attention == "valu"
    assert LN.CaptionMode("native", "torch", "native", False, "valu").decode_attention == "valu"       # five positionals go on working
    m = LN.CaptionMode(decode_attention="mfma")
    assert m.decode_attention == "mfma" and m != LN.CaptionMode() and m.decode == "valu"
    with pytest.raises(ValueError) as e:
        LN.CaptionMode(decode_attention="wmma")
    assert "decode_attention" in str(e.value) and str(LN.CAPTION_ATTENTIONS) in str(e.value)


def test_caption_mode_maps_the_fourth_switch():
    from rsvld_amd import llava_next as LN
    assert LN.caption_mode("e4m3", "flash", "mfma").decode_attention == "valu"                        # the three-value form
    assert LN.caption_mode("e4m3", "flash", "mfma") == LN.CaptionMode("e4m3", "flash", "native", False, "mfma")
    m = LN.caption_mode("e4m3-only", "flash", "mfma", "mfma")
    assert m == LN.CaptionMode("e4m3", "flash", "e4m3", True, "mfma", "mfma")
    assert LN.caption_mode(attention="mfma") == LN.CaptionMode(decode_attention="mfma")
    with pytest.raises(ValueError) as e:
        LN.caption_mode(None, None, None, "fast", who="somebody", names=("a", "b", "c", "their_attention"))
    assert "somebody" in str(e.value) and "their_attention" in str(e.value) and str(LN.CAPTION_ATTENTIONS) in str(e.value)
    with pytest.raises(ValueError) as e:                                                             # three names: the fourth has a default
        LN.caption_mode(None, None, None, "fast", names=("a", "b", "c"))
    assert "attention" in str(e.value)


def test_pipeline_config_and_both_parsers(tmp_path):
    from rsvld_amd import infer, infer_dir
    base = dict(input_img="a.png", output_dir=str(tmp_path / "o"))
    assert infer.PipelineConfig(**base).caption_attention == "valu"
    assert infer.PipelineConfig(**base, caption_attention="mfma").caption_attention == "mfma"
    with pytest.raises(ValueError) as e:
        infer.PipelineConfig(**base, caption_attention="bogus")
    assert "caption_attention" in str(e.value)
    for parser, argv in ((infer.build_parser(), ["--input_img", "a.png"]), (infer_dir.build_parser(), ["--image_dir", "a", "--save_dir", "b"])):
        assert parser.parse_args(argv).caption_attention == "valu"
        assert parser.parse_args(argv + ["--caption_attention", "mfma"]).caption_attention == "mfma"
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--caption_attention", "bogus"])


def test_wrappers_validate_kernel_before_anything_else():
    from rsvld_amd import decode_rows as DR, ops
    with pytest.raises(ValueError, match="kernel='wmma'"):
        DR.llama_decode_attention_rows(None, None, None, None, None, None, 8, 2, 1.0, kernel="wmma")
    with pytest.raises(ValueError, match="kernel='wmma'"):
        ops.llama_decode_attention(None, None, None, None, None, None, 8, 2, 1.0, kernel="wmma")


# ---- the plan and the workspace
def test_plan_range_keys_do_not_depend_on_max_len_and_it_takes_no_row_count():
    from rsvld_amd import _lib
    assert len(_lib.SIGNATURES["rsvld_plan_llama_decode_attention_mma"][1]) == 5        # n_q, n_kv, max_len, dtype, plan*: no B
    pls = {n: plan(32, 8, n) for n in (384, 3328, 8325)}
    R = pls[384].range_keys
    assert R % 64 == 0 and all(int(p.range_keys) == R for p in pls.values())
    for n, p in pls.items():
        assert p.ranges == -(-n // R) and (p.grid_x, p.grid_y) == (8, p.ranges) and p.waves * 32 == R and p.lds_bytes == 2 * R * 128 * 2
    for dt in CA.DTYPES:
        assert plan(32, 8, 3328, dt).range_keys == R
    lib = _lib.load()
    pl = _lib.DecodeAttentionMmaPlan()
    assert lib.rsvld_plan_llama_decode_attention_mma(9, 1, 384, _lib.F16, pl) == -2      # nine heads on one kv head
    assert lib.rsvld_plan_llama_decode_attention_mma(8, 3, 384, _lib.F16, pl) == -1
    assert lib.rsvld_plan_llama_decode_attention_mma(8, 2, 384, _lib.F16, None) == -1


def test_workspace_is_linear_in_the_sequences():
    from rsvld_amd import _lib
    ws = _lib.load().rsvld_llama_decode_attention_mma_rows_ws_bytes
    for n_q, n_kv, max_len in ((32, 8, 3328), (2, 1, 8325), (7, 1, 40)):
        one = int(ws(n_q, n_kv, max_len, 1))
        ranges = plan(n_q, n_kv, max_len).ranges
        assert one == n_q * (128 * 2 + ranges * 130 * 4)                                 # the rotated q in T, then the partials
        assert [int(ws(n_q, n_kv, max_len, B)) for B in range(1, 9)] == [B * one for B in range(1, 9)]
    assert ws(32, 8, 3328, 0) == 0 and ws(32, 8, 3328, 9) == 0


def test_entry_point_checks_before_any_launch():
    """Null pointers: whatever is wrong with the shape is said first, nothing is dereferenced or launched."""
    from rsvld_amd import _lib
    fn = _lib.load().rsvld_llama_decode_attention_mma_rows
    p = 256                                                                             # (a non-null, aligned address that is never used)
    call = lambda n_q, n_kv, hd, B: fn(p, p, p, p, p, p, p, p, n_q, n_kv, hd, 384, B, 1.0, _lib.F16, None)
    assert call(8, 2, 128, 9) == -1 and call(8, 2, 128, 0) == -1
    assert call(8, 2, 64, 1) == -2 and call(9, 1, 128, 1) == -2
    assert fn(p, p, p, p, p, p, p, None, 8, 2, 128, 384, 1, 1.0, _lib.F16, None) == -1
    assert fn(p, p, p, p, p, p, p, p + 4, 8, 2, 128, 384, 1, 1.0, _lib.F16, None) == -1    # a workspace that is not 16-byte aligned


def test_the_attention_kernels_use_no_scratch():
    """Both instantiations are there, with matrix instructions, and without a scratch instruction (tools/audit_scratch.py, as
    tests/test_build_audits.py uses it for the other LDS-DMA units)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import audit_scratch
    res = audit_scratch.audit("decode_attention.hip")
    assert len(res) == 2 and all("dam_kernel" in k for k in res), res
    assert not any(res.values()), res


# ---- the cases of the GPU test, on the CPU
def _cases(dtype):
    R = range_keys()
    for group in CA.DECODE_GROUPS:
        yield from CA.decode_cases(*group, positions(R), dtype, group in CA.DECODE_RAMP_GROUPS)


@_DT
def test_the_rounded_fp64_reference_passes_every_case_at_the_new_positions(dtype):
    worst, n = {}, 0
    for c in _cases(dtype):
        worst[c.family] = max(worst.get(c.family, 0.0), CA.check(c, CA.reference(c)))
        n += 1
    print(f"ideal kernel, {CA.DTN[dtype]}, {n} cases: worst ratio to the bound {worst}")
    assert n == len(positions(range_keys())) * (2 * len(CA.DECODE_GROUPS) + 2 * len(CA.DECODE_RAMP_GROUPS))
    assert worst["needle"] == 0.0 and worst["counting"] <= 0.5 and worst["ramp"] <= 0.5


@_DT
def test_needle_leak_at_the_new_positions(dtype):
    for c in _cases(dtype):
        if c.family == "needle":
            assert float(CA.needle_leak(c).max()) < CA.LEAK_BOUND, c.label


def _rejects(c, got):
    try:
        CA.check(c, got)
    except AssertionError:
        return True
    return False


@_DT
@pytest.mark.parametrize("fault", [1, 3, 4, 5, 6, 8], ids=lambda f: f"fault{f}")
def test_the_evaluators_faults_are_rejected_at_the_new_positions(fault, dtype):
    """A dropped key, the stale cache row as the new key, a key counted twice, V rows exchanged, heads exchanged, the missed rescale."""
    caught = next((c for c in _cases(dtype) if _rejects(c, CA.reference(c, fault=fault))), None)
    assert caught is not None, f"no case rejects: {CA.FAULTS[fault]}"
    print(f"fault {fault} ({CA.FAULTS[fault]}): rejected by {caught.label}")


def reference_without_keys(c, drop):
    """``CA.reference`` of the case with the keys ``drop`` (a set) never seen: the remaining keys of the row, in order."""
    keep = [j for j in range(c.pos + 1) if j not in drop]
    assert keep
    return CA.reference(types.SimpleNamespace(**{**vars(c), "k64": c.k64[:, keep], "v64": c.v64[:, keep], "positions": [len(keep) - 1]}))


def reference_with_q_of(c, other):
    """``CA.reference`` of the case on the rotated queries of ``other`` (the same group and dtype): the q buffer of another sequence."""
    assert other.q64.shape == c.q64.shape
    return CA.reference(types.SimpleNamespace(**{**vars(c), "q64": other.q64}))


@_DT
def test_the_last_key_of_a_range_dropped_is_rejected(dtype):
    R = range_keys()
    for c in CA.decode_cases(8, 2, [(384, p) for p in (R - 1, R, 2 * R - 1, 2 * R, 383)], dtype, False):
        last = {j for j in range(c.pos + 1) if j % R == R - 1}
        if c.family == "counting":
            assert _rejects(c, reference_without_keys(c, last)), c.label
        elif last & set(c.targets[0].tolist()):                      # a needle whose target is such a key
            assert _rejects(c, reference_without_keys(c, last)), c.label
    c = CA.needle_decode(8, 2, 384, R - 1, 0, dtype)                 # family "p": the row's own key is the last of range 0
    assert R - 1 in c.targets[0].tolist() and _rejects(c, reference_without_keys(c, {R - 1}))


@_DT
@pytest.mark.parametrize("wave", range(4))
def test_a_waves_partial_dropped_in_the_merge_is_rejected(dtype, wave):
    """Wave w of a range's workgroup holds keys 32 w .. 32 w + 31 of the range: dropped in range 0 and in range 1."""
    R = range_keys()
    per = R // 4
    for pos, base in ((R - 1, 0), (2 * R - 1, R), (383, R)):
        drop = set(range(base + per * wave, base + per * (wave + 1)))
        c = CA.counting_decode(8, 2, 384, pos, dtype)
        assert _rejects(c, reference_without_keys(c, drop)), (pos, base)
        r = CA.ramp_decode(8, 2, 384, pos, dtype, "saw")
        assert _rejects(r, reference_without_keys(r, drop)), (pos, base)


@_DT
def test_the_rotated_q_of_another_sequence_is_rejected(dtype):
    R = range_keys()
    a, b = (CA.needle_decode(8, 2, 384, p, t, dtype) for t, p in enumerate((R + 1, 2 * R - 1)))
    assert _rejects(a, reference_with_q_of(a, b)) and _rejects(b, reference_with_q_of(b, a))
    ra, rb = CA.ramp_decode(8, 2, 384, R + 1, dtype, "up"), CA.ramp_decode(8, 2, 384, 2 * R - 1, dtype, "up")
    assert _rejects(ra, reference_with_q_of(ra, rb))


@_DT
def test_the_combine_cases_of_66_ranges_are_fair(dtype):
    R = range_keys()
    max_len, pos = combine_shape(R)
    assert plan(*CA.COMBINE_GROUP, max_len).ranges == 66
    for c in CA.decode_cases(*CA.COMBINE_GROUP, [(max_len, p) for p in pos], dtype, True):
        CA.check(c, CA.reference(c))
