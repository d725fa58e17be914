"""The case tables of tests/test_gpu_matrix_exact.py, walked on the CPU: the exact cases rest on properties of their INPUTS (the
fp64 reference is representable at every epilogue step, fp32 and fp64 references agree, no fp32 partial sum can round, tile sums
stay below 2^24) and on shape arithmetic (which instantiation a row lands in).  Both are checked here for every row, GPU or not:
the builders assert the first kind; the second is the answer of the library's own planner (rsvld_plan_conv: host code, no device) about
the row's descriptor, so these tests need the built library as tests/test_cabi.py does."""
import itertools
import re
from pathlib import Path

import pytest
import torch

import test_gpu_matrix_exact as MX

F16, BF16 = torch.float16, torch.bfloat16
CSRC = Path(__file__).resolve().parents[1] / "remote-sensing-vision-language-diffusion-model_amd" / "csrc"


def _routes(row, s, dtype=0, out_f32=0):
    return MX.planned_inst(MX.conv_desc(s, row.tune, dtype, out_f32))


@pytest.mark.parametrize("dtype", MX.DTYPES, ids=MX._DTN.get)
@pytest.mark.parametrize("row", MX.ROWS, ids=MX._ids(MX.ROWS))
def test_row_inputs_are_exact_and_route_as_claimed(dtype, row):
    sa = row.a_shape
    assert _routes(row, sa) == row.inst
    ca = MX.build_conv_exact(dtype, sa, "A")          # asserts the input-side conditions
    Ho, Wo, M, kc = MX.geometry(sa)
    assert ca["want"].shape == (sa.B, Ho, Wo, sa.Cout)
    # ragged everywhere: M against the tile's rows, Cout against its columns, a partial last K step, a seam inside a K step
    assert M % row.inst.bm and M > row.inst.bm and sa.Cout % row.inst.bn and kc % 8 and sa.C1 % 64
    if row.inst.ks == 2:
        nk = MX.nk_of(sa)
        assert nk >= 17 and nk % 2 == 1
    if row.b is None:
        return
    sb = MX.shape_b(row.cout, *row.b)
    assert _routes(row, sb) == row.inst
    cb = MX.build_conv_exact(dtype, sb, "B")
    assert cb["res"] is None and MX.geometry(sb)[2] % row.inst.bm
    for geglu in (False, True):
        st = MX.shape_a(32 if (geglu and row.cout == 24) else row.cout)._replace(C1=120, C2=0)
        assert _routes(row, st) == row.inst
    assert row.label == f"conv_igemm_{row.inst.bm}x{row.inst.bn}"       # the label of ops.conv2d names the tile that runs


def test_case_b_alternates_and_holds_the_1x1_rows():
    modes = [r.b[0] for r in MX.SMALL_ROWS]
    assert modes.count("s2") == len(modes) // 2 and modes.count("up") == len(modes) // 2
    one = {(r.inst.bm, r.inst.bn) for r in MX.SMALL_ROWS if r.b[1] == 1}
    assert {(64, 64), (128, 128)} <= one


def test_every_instantiation_of_both_dispatch_functions_has_a_row():
    """The launch tables -- CONV_TABLE of csrc/conv_igemm.hip, launch_plan of csrc/conv_halo.hip: the only places an instantiation is
    named -- against the rows; the multi-segment rows cover every LDS-DMA tile family.  And the planner against the tables: over the
    tune words of ROWS it reaches every entry and returns nothing else."""
    src = (CSRC / "conv_igemm.hip").read_text()
    body = src[src.index("#define CONV_TABLE(X)"):src.index("int launch_plan(")]
    want = {MX.Inst(int(m[1]), int(m[2]), int(m[4]), int(m[5]), "lds" if m[3] == "true" else "reg")
            for m in re.finditer(r"X\((\d+), (\d+), \d, \d, (true|false), (\d), (\d)\)", body)}
    assert len(re.findall(r"launch_conv<", src)) == 1, "an instantiation is named outside the table"
    have = {r.inst for r in MX.ROWS}
    assert want == have, (want - have, have - want)
    assert len(have) == 19
    assert {(r.inst.bm, r.inst.bn) for r in MX.SEG_ROWS} == {(i.bm, i.bn) for i in have if i.staging == "lds"} - {(256, 64)}
    hsrc = (CSRC / "conv_halo.hip").read_text()
    hbody = hsrc[hsrc.index("int launch_plan("):hsrc.index("rsvld_conv3x3_halo_supported")]
    hwant = {(64, 4)} if "launch_halo<T, 64, 4, 2>" in hbody else set()
    hwant |= {(int(m[1]), int(m[2])) for m in re.finditer(r"launch_halo32<T, (\d+), (\d)>", hbody)}
    assert hwant == {r.inst for r in MX.HALO_ROWS} and len(hwant) == 3
    assert len(re.findall(r"launch_halo(?:32)?<T, \d", hsrc)) == 3, "an instantiation is named outside the table"
    # the planner over rows, channel widths, K depths and every tune word of the tables
    tunes = sorted({r.tune for r in MX.ROWS} | {r.tune for r in MX.SEG_ROWS})
    seen = set()
    for (M, k), cout, c1, tune in itertools.product(((297, 3), (8316, 3), (8190, 3), (16380, 3), (360, 1), (70000, 1)), (8, 24, 32, 48, 64, 72, 176, 320),
                                                    (24, 120, 1032), tunes):
        seen.add(MX.planned_inst(MX.conv_desc(MX.Shape(1, 1, M, c1, 0, cout, k, "p1"), tune)))
    assert seen == want, (want - seen, seen - want)
    hseen = set()
    for (B, H, W), cout, cin, row in itertools.product(((2, 19, 45), (1, 27, 45), (4, 512, 512)), (8, 48, 64, 72, 192), (64, 192), MX.HALO_ROWS + [None]):
        p = MX.plan_conv(MX.conv_desc(MX.Shape(B, H, W, cin, 0, cout, 3, "p1"), row.tune if row else 0))
        hseen.add((p.halo_bn, p.halo_waves))
    assert hseen == hwant, hseen


@pytest.mark.parametrize("side", MX.SEG_SIDES)
@pytest.mark.parametrize("mode", list(MX.SEG_MODES))
@pytest.mark.parametrize("row", MX.SEG_ROWS, ids=MX._ids(MX.SEG_ROWS))
def test_multi_segment_inputs_are_exact_and_route_as_claimed(row, mode, side):
    c = MX.build_seg_exact(mode, side, row.cout)
    from rsvld_amd import _lib as L
    assert _routes(row, c["s"], {"split3": L.SPLIT, "pair2": L.F16W2, "w1": L.F16W1}[mode], 1) == row.inst
    lo = c["x"] if side == "xlo" else c["w"]
    assert not torch.equal(lo, lo.round())            # the low part is there ...
    other = c["w"] if side == "xlo" else c["x"]
    assert torch.equal(other, other.round())          # ... on one side only


@pytest.mark.parametrize("dtype", MX.DTYPES, ids=MX._DTN.get)
@pytest.mark.parametrize("hs", **MX._HS)
@pytest.mark.parametrize("row", MX.HALO_ROWS, ids=MX._ids(MX.HALO_ROWS))
def test_halo_inputs_are_exact_and_route_as_claimed(dtype, row, hs):
    B, H, W, C1, C2 = hs
    cp = (row.cout + 7) // 8 * 8
    plan = MX.plan_conv(MX.conv_desc(MX.Shape(B, H, W, C1, C2, row.cout, 3, "p1"), row.tune, cout_p=cp))
    assert (plan.halo_bn, plan.halo_waves) == row.inst and row.label == f"conv_halo_{plan.halo_bn}"
    assert cp != row.cout and cp % row.inst[0]        # pad channels, ragged column tile
    assert H % 16 and H % 8 and W % 32                # ragged last tile row (8- and 16-row tiles) and column
    c = MX.build_halo_exact(dtype, row.cout, hs)      # asserts integer tile sums below 2^24
    assert c["part"].shape == (B, (H + 7) // 8 * 2, cp, 2) == (B, plan.halo_stat_tiles, cp, 2)
    assert float(c["part"][:, :, row.cout:].abs().max()) == 0.0
    # the reference partials add up to the whole tensor's sums
    assert torch.equal(c["part"].sum(1)[..., 0], c["want"].sum((1, 2)))


def test_fp32_out_case_is_exact():
    for dtype in MX.DTYPES:
        c = MX.build_f32_out_exact(dtype)
        assert MX.planned_inst(MX.conv_desc(c["s"], 0, out_f32=1, cout_p=8)).bn == 32


@pytest.mark.parametrize("dtype", MX.DTYPES, ids=MX._DTN.get)
@pytest.mark.parametrize("case", MX.GEMM_ROWS, ids=[n for n, _ in MX.GEMM_ROWS])
def test_gemm_rows(dtype, case):
    """Operand ranges and the reference of a 256-row slice (the whole references are computed where the GPU tests run)."""
    name, (M, K, N) = case
    form = lambda tune: MX.plan_conv(MX.linear_desc(M, K, N, tune)).gemm256       # 1: persistent where a device is, 2: one tile, 0: not taken
    assert form(0) == 1 and form(MX.ONE_TILE) == 2 and form(MX.NO_GEMM256) == 0
    whole, halves = MX.persistent_tiles(M, N)
    assert {"whole_tiles": halves == 0 and N % 256 == 0, "half_tile_round": halves == 8 * 26, "ragged_n_tile": N % 256 == 8}[name]
    inst = MX.planned_inst(MX.linear_desc(M, K, N, MX.NO_GEMM256))
    assert (inst.bm, inst.bn) == (128, 128)
    o = MX.build_gemm_operands(dtype, M, K, N)
    want = MX.gemm_reference(dtype, o, rows=256)
    assert want.shape == (256, N)
