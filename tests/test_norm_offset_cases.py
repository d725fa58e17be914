"""The case tables of tests/test_gpu_norm_offset.py, walked on the CPU (tests/norm_offset_cases.py): every case must be FAIR (ideal
statistics through the kernels' own fp32 affine and output rounding stay within half the bound the GPU test applies), must land in
the route it names (the library's planner, rsvld_plan_groupnorm), and must have TEETH (fp32 (sum, sum of squares) partials in
gn_partial_kernel's order, the arithmetic these kernels had, break the fp32-input bound at mean / sigma = 64)."""
import pytest
import torch

import norm_offset_cases as NC

F16, BF16, F32 = NC.F16, NC.BF16, NC.F32
SHAPES = NC.GN_SHAPES + [NC.WIDE_SHAPE]


def _outs(dtype):
    return [(dtype, NC.gn_bound(dtype))] if dtype != F32 else [("f32", NC.SPLIT_F32_OUT), ("planes", NC.SPLIT_PLANES_OUT)]


def test_ladder_tops_are_where_the_type_resolves_sigma_into_16_steps():
    for dt, p in NC.SIGNIFICAND.items():
        assert max(NC.LADDER[dt] + NC.VAR_ONLY[dt]) <= 2 ** (p - 4)
    assert max(NC.LADDER[F16]) == 2 ** (11 - 4) and max(NC.LADDER[BF16]) == 2 ** (8 - 4)


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=NC.DTN.get)
@pytest.mark.parametrize("s", SHAPES, ids=[s.name for s in SHAPES])
def test_group_norm_cases_are_fair(s, dtype):
    if s.name == "wide" and dtype != F32:
        return                                            # an fp32-input case only
    for R in NC.LADDER[dtype]:
        c = NC.gn_case(s.name, dtype, R)
        # the generator did what it says: every group sits R sigma from zero, with unit spread
        ratio = c["mean"].abs() / c["var"].sqrt()
        assert float((ratio / R - 1).abs().max()) < 0.1, (R, ratio)
        assert torch.equal(c["x"], c["x"].to(dtype).float())
        for out, bound in _outs(dtype):
            e = NC.ideal_gn_error(c, out)
            print(f"{s.name} {NC.DTN[dtype]} R={R} out={out}: ideal affine {e:.2e} of range (bound {bound:.0e})")
            assert e <= 0.5 * bound, (s.name, dtype, R, out, e)
    c = NC.gn_case(s.name, dtype, max(NC.LADDER[dtype]), *NC.SMALL_SIGMA)
    for out, bound in _outs(dtype):
        assert NC.ideal_gn_error(c, out) <= 0.5 * bound


def test_fp32_family_case_is_fair_and_512_is_not():
    for R in NC.LADDER[F32]:
        assert NC.ideal_gn_error(NC.gn_case("family", F32, R), "f32") <= 0.5 * NC.F32_FAMILY
    assert NC.ideal_gn_error(NC.gn_case("family", F32, max(NC.LADDER[F32]), *NC.SMALL_SIGMA), "f32") <= 0.5 * NC.F32_FAMILY
    with pytest.raises(KeyError):
        NC.gn_case("famly", F32, 8)                       # no silent stand-in for a mistyped name
    # the rung kept for the statistics alone: an ideal fp32 affine is already near the output bounds there
    e = NC.ideal_gn_error(NC.gn_case("gs2", F32, 512), "f32")
    print(f"fp32 R=512: ideal affine {e:.2e} of range")
    assert e > 0.5 * NC.SPLIT_F32_OUT


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=NC.DTN.get)
@pytest.mark.parametrize("rows,C", NC.LN_SHAPES)
def test_layer_norm_cases_are_fair(rows, C, dtype):
    outs = [(dtype, NC.TOL16[dtype])] if dtype != F32 else [("f32", NC.F32_FAMILY), ("f32", NC.SPLIT_LN_F32_OUT), ("planes", NC.SPLIT_LN_PLANES_OUT)]
    for R, sigma in [(R, 1.0) for R in NC.LADDER[dtype]] + [(max(NC.LADDER[dtype]), NC.SMALL_SIGMA[0])]:
        c = NC.ln_case(rows, C, dtype, R, sigma)
        assert torch.equal(c["x"], c["x"].to(dtype).float())
        for out, bound in outs:
            e = NC.ideal_ln_error(c, out)
            print(f"layer_norm {rows}x{C} {NC.DTN[dtype]} R={R} sigma={sigma} out={out}: ideal {e:.2e} of range (bound {bound:.0e})")
            assert e <= 0.5 * bound


def _epi_cases():
    out = [(NC.EPI16[t], dt, False, NC.TOL16[dt], dt, f"{t}-{NC.DTN[dt]}") for t in NC.EPI16 for dt in (F16, BF16)]
    # the consumer of an fp32 producer normalises into planes (rsvld_groupnorm_apply_split in front of the split convolution)
    return out + [(geo, F16 if m == "pair2" else F32, m == "q8", NC.SPLIT_PLANES_OUT, "planes", m) for m, (geo, _) in NC.EPI32.items()]


@pytest.mark.parametrize("geo,dtype,pre_norm,bound,out,name", _epi_cases(), ids=[c[-1] for c in _epi_cases()])
def test_epilogue_cases_are_fair(geo, dtype, pre_norm, bound, out, name):
    """The consumer's GroupNorm over the producer's output (computed here in fp32 on the CPU): the offset reaches it, at the stated
    spread, and ideal statistics through the fp32 affine stay within half the consumer norm's bound."""
    ladder = NC.LADDER[F32] if out == "planes" else NC.LADDER[dtype]
    for R, sigma in [(R, 1.0) for R in ladder] + [(max(ladder), NC.SMALL_SIGMA[0])]:
        c = NC.producer_case(geo, R, sigma, dtype, pre_norm)
        x = c["stored"]
        xg = x.double().reshape(x.shape[0], NC.EPI_GROUPS, -1)
        ratio = xg.mean(-1).abs() / xg.std(-1)
        assert float((ratio / R - 1).abs().max()) < 0.2 and abs(float(xg.std(-1).mean()) / sigma - 1) < 0.2, (R, sigma)
        e = NC.ideal_gn_error_of(x, c["gamma"], c["beta"], NC.EPI_GROUPS, NC.EPI_EPS, out)
        print(f"epilogue {name} R={R} sigma={sigma}: ideal affine {e:.2e} of range (bound {bound:.0e})")
        assert e <= 0.5 * bound


def test_cases_land_in_the_routes_they_name():
    for s in NC.GN_SHAPES:
        HW = s.H * s.W
        for dt in (F16, BF16):
            assert NC.gn_route(dt, HW, s.C1, s.C2, s.groups) == s.route16, s.name
        assert NC.gn_route(F32, HW, s.C1, s.C2, s.groups) == "partial"
        assert (s.C1 + s.C2) % s.groups == 0 and s.C1 % 8 == 0 and s.C2 % 8 == 0
    by = NC.GN_BY_NAME
    w = NC.WIDE_SHAPE                                                     # sums + pivots above 64 KiB of LDS, sums alone below
    rif = NC.gn_plan(F32, w.B, w.H * w.W, w.C1, 0, w.groups).rows_in_flight
    assert rif * w.C1 * 8 <= 65536 < rif * w.C1 * 8 + w.C1 * 4
    assert NC.gn_route(F32, w.H * w.W, w.C1, 0, w.groups) == "partial"

    def chunks(HW):                                                       # the chunking depends on the image size alone
        p = NC.gn_plan(F32, 1, HW, 64, 0, 32)
        return p.nchunks, p.rows_per_chunk

    assert chunks(48 * 48) == (36, 64) and chunks(9 * 33) == (5, 64) and 9 * 33 % 64 == 41
    assert chunks(512 * 512) == (512, 512)                                # a chunk is 512 rows
    assert chunks(19 * 23)[0] > 1                                         # more than one block on the partial route too
    st = by["straddle"]
    gs = (st.C1 + st.C2) // st.groups
    assert st.C1 % gs != 0 and gs % 8 != 0                                # a group lies across the two sources, and across vectors
    assert (by["gs2"].C1 // by["gs2"].groups) == 2
    # the odd sizes: rows that are no multiple of the rows in flight
    assert (19 * 23) % 32 and (9 * 33) % 32


def test_fp32_sum_sumsq_partials_break_the_fp32_input_bound_at_64():
    """Teeth: the arithmetic the statistics pass had -- fp32 (sum, sum of squares) per thread and per block, fp64 only across chunks --
    misses the split precision's GroupNorm bound at mean / sigma = 64 and the variance bound with it; at 8 it does not (so the cases
    see the defect, not the shape).  The pivoted sums that replace it stay at the ideal figure on every rung, 512 included."""
    fig = {}
    for R in (8, 64, 512):
        c = NC.gn_case("gs2", F32, R)
        s = c["s"]
        for name, emu in (("fp32 pair", NC.emulate_partial_sums_fp32), ("pivot", NC.emulate_partial_sums_pivot)):
            mean, var = emu(c)
            em, ev = NC.stats_errors(mean, var, c)
            y = NC.affine_from_stats(c["x"], mean.float(), var.float(), c["gamma"], c["beta"], s.groups, c["eps"])
            fig[name, R] = (em, ev, NC.rel_err(y, c["want"]))
            print(f"{name:9s} R={R:3d}: mean {em:.2e} sigma, variance {ev:.2e} relative, output {fig[name, R][2]:.2e} of range")
    bound = NC.SPLIT_F32_OUT
    assert fig["fp32 pair", 8][2] <= bound and fig["fp32 pair", 8][1] <= 2 * bound
    assert fig["fp32 pair", 64][2] > bound and fig["fp32 pair", 64][1] > 2 * bound
    assert fig["fp32 pair", 512][1] > 100 * bound
    for R in (8, 64):
        assert fig["pivot", R][2] <= 0.5 * bound
    for R in (8, 64, 512):
        assert fig["pivot", R][1] <= bound and fig["pivot", R][0] <= bound      # half the GPU test's 2 x bound; bound x sigma
