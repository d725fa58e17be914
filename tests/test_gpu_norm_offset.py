"""GroupNorm / LayerNorm on offset-dominated inputs (tests/norm_offset_cases.py: every group sits at +-R sigma), every statistics
route through rsvld_amd.ops against F.group_norm / F.layer_norm of the same values in fp64, at the bounds the routes' own tests
already assert.  Where a route exposes its statistics: variance relative error per group <= 2 x the route's output bound (a relative
error d in the variance moves each normalised value by d / 2 of itself), mean error <= the output bound x sigma.
The CPU half (fairness of every case, the routes, the emulation of the fp32 (sum, sumsq) arithmetic this file was written against)
is tests/test_norm_offset_cases.py.  Measured figures are printed."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_offset_cases as NC

pytestmark = pytest.mark.gpu
F16, BF16, F32 = NC.F16, NC.BF16, NC.F32


def _rungs(dtype, var_only=False):
    """(R, sigma, eps, outputs checked) of a storage type: its ladder at unit spread, one small-spread case at the top rung, and the
    rungs where only the statistics are checked."""
    r = [(R,) + NC.UNIT + (True,) for R in NC.LADDER[dtype]] + [(max(NC.LADDER[dtype]),) + NC.SMALL_SIGMA + (True,)]
    if var_only:
        r += [(R,) + NC.UNIT + (False,) for R in NC.VAR_ONLY[dtype]]
    return r


def _params(dtypes, names, var_only=False):
    out, ids = [], []
    for n in names:
        for dt in dtypes:
            for rung in _rungs(dt, var_only):
                out.append((n, dt, rung))
                ids.append(f"{n}-{NC.DTN[dt]}-R{rung[0]}" + ("-s0.05" if rung[1] != 1.0 else "") + ("" if rung[3] else "-var"))
    return dict(argnames="name,dtype,rung", argvalues=out, ids=ids)


def _nhwc(x, dev, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def _sources(c, dev):
    s, dt = c["s"], c["dtype"]
    return _nhwc(c["x"][:, :s.C1], dev, dt), (_nhwc(c["x"][:, s.C1:], dev, dt) if s.C2 else None)


def _cmp(got, want, bound, what):
    """max |got - want| against ``bound`` of want's range (both NCHW, or any common layout)"""
    got, want = got.double().cpu(), want.double()
    s = float(want.abs().max())
    e = float((got - want).abs().max())
    print(f"{what}: max|d| = {e:.3e} (range {s:.2f}, rel {e / max(s, 1e-30):.2e}, bound {bound:.0e})")
    assert e <= bound * max(s, 1e-6), f"{what}: max|d| = {e:.3e}, range {s:.3e}, bound {bound:.0e} of range"


def _cmp_stats(st, c, bound, what, means=True):
    """(mean, biased variance) rows [B, groups, 2] against the fp64 ones"""
    st = st.double().cpu()
    em, ev = NC.stats_errors(st[..., 0], st[..., 1], c)
    print(f"{what}: mean off by {em:.2e} sigma, variance by {ev:.2e} relative (bounds {bound:.0e}, {2 * bound:.0e})")
    assert ev <= 2 * bound, f"{what}: variance relative error {ev:.3e} > {2 * bound:.0e}"
    if means:
        assert em <= bound, f"{what}: mean error {em:.3e} sigma > {bound:.0e}"


def _ref_stats(c, dev):
    return torch.stack([c["mean"], c["var"]], -1).float().to(dev)


def _conv_after_norm(c, cout, seed):
    """A 3x3 convolution behind GroupNorm + SiLU of the case: weights of the case's storage type, the fp64 reference."""
    s, dt = c["s"], c["dtype"]
    C = s.C1 + s.C2
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, C, 3, 3, generator=g) / math.sqrt(9 * C)
    w = w if dt == F32 else w.to(dt).float()
    want = F.conv2d(F.silu(c["want"]), w.double(), None, padding=1)
    return w, want


# ---------------------------------------------------------------------------------------------------------------------------------
# 16-bit routes: the one-workgroup kernel (shape "small") and the row-chunk partials (the others)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**_params((F16, BF16), [s.name for s in NC.GN_SHAPES]))
def test_group_norm_16bit(cuda, name, dtype, rung):
    """rsvld_groupnorm_nhwc, rsvld_groupnorm_stats, rsvld_groupnorm_apply with supplied statistics, and rsvld_groupnorm_scale_shift
    in front of the fused convolution (conv2d(norm=))"""
    from rsvld_amd import ops
    R, sigma, eps, _ = rung
    c = NC.gn_case(name, dtype, R, sigma, eps)
    s, bound = c["s"], NC.gn_bound(dtype)
    tag = f"{name} {NC.DTN[dtype]} R={R} sigma={sigma}"
    x1, x2 = _sources(c, cuda)
    ga, be = c["gamma"].to(cuda), c["beta"].to(cuda)
    got = ops.group_norm(x1, ga, be, s.groups, eps, x2=x2)
    assert got.dtype == dtype
    _cmp(got.permute(0, 3, 1, 2), c["want"], bound, f"group_norm [{s.route16}] {tag}")
    _cmp_stats(ops.group_norm_stats(x1, s.groups, x2=x2), c, bound, f"  group_norm_stats {tag}")
    got2 = ops.group_norm_apply(x1, _ref_stats(c, cuda), ga, be, s.groups, eps, x2=x2)
    _cmp(got2.permute(0, 3, 1, 2), c["want"], bound, f"  group_norm_apply, supplied statistics {tag}")
    if s.C1 % 64 or s.C2 % 64:
        return
    w, want = _conv_after_norm(c, 64, 5)
    with ops.tuning(halo_min_wgs=0, profiler=(prof := ops.LaunchProfiler())):
        y = ops.conv2d(x1, ops.pack_conv(w, None, dtype, cuda), x2=x2, pad=1, norm=(ga, be, s.groups, eps, True))
    names = set(prof.summary())
    assert "groupnorm_stats(3 kernels)" in names and any(n.startswith("conv_halo") for n in names), names
    _cmp(y.permute(0, 3, 1, 2), want, bound, f"  conv2d(norm=) {tag}")


SPREADS = dict(argnames="spread", argvalues=[NC.UNIT, NC.SMALL_SIGMA], ids=["s1", "s0.05"])


@pytest.mark.parametrize(**SPREADS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=NC.DTN.get)
def test_group_norm_modulated_16bit(cuda, dtype, spread):
    """ZeroSFT: norm(x) (1 + scale) + shift, the modulation two channel slices of one stacked tensor; statistics from the partials.
    (Fairness of the case: the GroupNorm of shape gs2 at this rung, tests/test_norm_offset_cases.py.)"""
    from rsvld_amd import ops
    R = max(NC.LADDER[dtype])
    c = NC.gn_case("gs2", dtype, R, *spread)
    s = c["s"]
    C = s.C1
    g = torch.Generator().manual_seed(11)
    mod = (torch.randn(s.B, s.H, s.W, 2 * C, generator=g) * 0.5).to(dtype)
    m64 = mod.double().permute(0, 3, 1, 2)
    want = c["want"] * (1 + m64[:, :C]) + m64[:, C:]
    md = mod.to(cuda)
    x1, _ = _sources(c, cuda)
    got = ops.group_norm(x1, c["gamma"].to(cuda), c["beta"].to(cuda), s.groups, c["eps"], mod_scale1p=md[..., :C], mod_shift=md[..., C:])
    _cmp(got.permute(0, 3, 1, 2), want, NC.gn_bound(dtype), f"group_norm modulated {NC.DTN[dtype]} R={R} sigma={spread[0]}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32-input routes of the split precision (ops.ALL_SPLIT): always the row-chunk partials
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**_params((F32,), [s.name for s in NC.GN_SHAPES] + ["wide"], var_only=True))
def test_group_norm_split(cuda, name, dtype, rung):
    """rsvld_groupnorm_scale_shift_f32 + rsvld_groupnorm_apply_split (fp32 and planes out, and in front of a convolution),
    rsvld_groupnorm_stats_f32_fast (one and two sources), rsvld_groupnorm_scale_shift_from_stats with supplied statistics"""
    from rsvld_amd import ops
    R, sigma, eps, outputs = rung
    c = NC.gn_case(name, F32, R, sigma, eps)
    s = c["s"]
    tag = f"{name} split R={R} sigma={sigma}"
    x1, x2 = _sources(c, cuda)
    ga, be = c["gamma"].to(cuda), c["beta"].to(cuda)
    with ops.f32_split(ops.ALL_SPLIT):
        st = ops.group_norm_stats(x1, s.groups, x2=x2)
        _cmp_stats(st, c, NC.SPLIT_F32_OUT, f"group_norm_stats (split) {tag}", means=outputs)
        if not outputs:
            return
        got = ops.group_norm(x1, ga, be, s.groups, eps, x2=x2)
        gp = ops.group_norm(x1, ga, be, s.groups, eps, x2=x2, planes=True)
        got2 = ops.group_norm_apply(x1, _ref_stats(c, cuda), ga, be, s.groups, eps, x2=x2)
        assert got.dtype == F32 and isinstance(gp, ops.Planes)
        _cmp(got.permute(0, 3, 1, 2), c["want"], NC.SPLIT_F32_OUT, f"  group_norm fp32 out {tag}")
        _cmp(gp.f32().permute(0, 3, 1, 2), c["want"], NC.SPLIT_PLANES_OUT, f"  group_norm planes out {tag}")
        _cmp(got2.permute(0, 3, 1, 2), c["want"], NC.SPLIT_F32_OUT, f"  group_norm_apply, supplied statistics {tag}")
        if s.C1 % 64 or s.C2 % 64 or name == "wide":
            return
        w, want = _conv_after_norm(c, 64, 5)
        pc = ops.pack_conv(w, None, F32, cuda, cin_split=(s.C1, s.C2) if s.C2 else None)
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            y = ops.conv2d(x1, pc, x2=x2, pad=1, norm=(ga, be, s.groups, eps, True))
        assert "groupnorm_stats_split" in set(prof.summary())
        _cmp(y.permute(0, 3, 1, 2), want, NC.SPLIT_CONV, f"  conv2d(norm=) {tag}")


@pytest.mark.parametrize(**SPREADS)
def test_group_norm_split_modulated(cuda, spread):
    from rsvld_amd import ops
    R = max(NC.LADDER[F32])
    c = NC.gn_case("gs2", F32, R, *spread)
    s = c["s"]
    C = s.C1
    g = torch.Generator().manual_seed(12)
    mod = torch.randn(s.B, s.H, s.W, 2 * C, generator=g) * 0.5
    m64 = mod.double().permute(0, 3, 1, 2)
    want = c["want"] * (1 + m64[:, :C]) + m64[:, C:]
    md = mod.to(cuda)
    x1, _ = _sources(c, cuda)
    with ops.f32_split(ops.ALL_SPLIT):
        got = ops.group_norm(x1, c["gamma"].to(cuda), c["beta"].to(cuda), s.groups, c["eps"], mod_scale1p=md[..., :C], mod_shift=md[..., C:])
    _cmp(got.permute(0, 3, 1, 2), want, NC.SPLIT_F32_OUT, f"group_norm split, modulated R={R} sigma={spread[0]}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 family (csrc/f32.hip): fp64 partial sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**_params((F32,), ["family"], var_only=True))
def test_group_norm_f32_family(cuda, name, dtype, rung):
    from rsvld_amd import ops
    R, sigma, eps, outputs = rung
    c = NC.gn_case(name, F32, R, sigma, eps)
    s = c["s"]
    tag = f"fp32 family R={R} sigma={sigma}"
    x1, _ = _sources(c, cuda)
    ga, be = c["gamma"].to(cuda), c["beta"].to(cuda)
    _cmp_stats(ops.group_norm_stats(x1, s.groups), c, NC.F32_FAMILY, f"group_norm_stats_f32 {tag}", means=outputs)
    if not outputs:
        return
    _cmp(ops.group_norm(x1, ga, be, s.groups, eps).permute(0, 3, 1, 2), c["want"], NC.F32_FAMILY, f"  group_norm_f32 {tag}")
    got2 = ops.group_norm_apply(x1, _ref_stats(c, cuda), ga, be, s.groups, eps)
    _cmp(got2.permute(0, 3, 1, 2), c["want"], NC.F32_FAMILY, f"  group_norm_apply_f32, supplied statistics {tag}")


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue partials: a producer convolution with stats=True whose bias is +-R per group of the consumer's GroupNorm (this is how an
# offset reaches a partial), then the consumer conv2d(norm=) on its output -- with the producer's partials, with a clone (statistics
# pass), and GroupNorm + SiLU + convolution of the producer's STORED output in fp64
# ---------------------------------------------------------------------------------------------------------------------------------
def _stats_of_partials(part, stored_nhwc, groups):
    """(mean, var) [B, groups] from the epilogue's per-tile per-channel (sum, sumsq), merged on the host in fp64, and the same from
    the stored tensor"""
    B, H, W, C = stored_nhwc.shape
    n = H * W * (C // groups)
    p = part.double().cpu().sum(1).reshape(B, groups, C // groups, 2).sum(2)
    mean = p[..., 0] / n
    var = p[..., 1] / n - mean * mean
    xg = stored_nhwc.double().cpu().permute(0, 3, 1, 2).reshape(B, groups, -1)
    return mean, var, xg.mean(-1), xg.var(-1, unbiased=False)


def _cmp_partials(part, stored, groups, bound, what, means=True):
    mean, var, rmean, rvar = _stats_of_partials(part, stored, groups)
    ev = float(((var - rvar).abs() / rvar).max())
    em = float(((mean - rmean).abs() / rvar.sqrt()).max())
    print(f"{what}: merged partials: mean off by {em:.2e} sigma, variance by {ev:.2e} relative (bounds {bound:.0e}, {2 * bound:.0e})")
    assert ev <= 2 * bound, f"{what}: variance relative error {ev:.3e} > {2 * bound:.0e}"
    if means:
        assert em <= bound, f"{what}: mean error {em:.3e} sigma > {bound:.0e}"


def _epi_ids(sigma, R, outputs=True):
    return f"R{R}" + ("-s0.05" if sigma != 1.0 else "") + ("" if outputs else "-var")


def _epi16_params():
    out, ids = [], []
    for tile in NC.EPI16:
        for dt in (F16, BF16):
            for R, sigma in NC.epi_rungs(dt):
                out.append((tile, dt, R, sigma))
                ids.append(f"{tile}-{NC.DTN[dt]}-" + _epi_ids(sigma, R))
    return dict(argnames="tile,dtype,R,sigma", argvalues=out, ids=ids)


@pytest.mark.parametrize(**_epi16_params())
def test_epilogue_partials_16bit(cuda, tile, dtype, R, sigma):
    from rsvld_amd import _lib as L, ops
    B, Cin, Cout, H, W = NC.EPI16[tile]
    c = NC.producer_case(NC.EPI16[tile], R, sigma, dtype)
    gamma, beta, wc = c["gamma"], c["beta"], c["wc"]
    bound = NC.gn_bound(dtype)
    norm = (gamma.to(cuda), beta.to(cuda), NC.EPI_GROUPS, NC.EPI_EPS, True)
    pcc = ops.pack_conv(wc, None, dtype, cuda)
    force = L.TUNE_HALO_NW8 if tile == "8wave" else L.TUNE_HALO_NW4
    with ops.tuning(halo_min_wgs=0, tune=ops.context().tune | force):
        ya = ops.conv2d(_nhwc(c["x"], cuda, dtype), ops.pack_conv(c["w"], c["bias"], dtype, cuda), pad=1, stats=True)
        assert hasattr(ya, "_gn_part")
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            got = ops.conv2d(ya, pcc, pad=1, norm=norm)            # statistics from the producer's epilogue
        assert "groupnorm_ab_from_partials" in set(prof.summary())
        ref = ops.conv2d(ya.clone(), pcc, pad=1, norm=norm)        # statistics pass over the tensor
    stored = ya.double().cpu().permute(0, 3, 1, 2)
    ratio = stored.reshape(B, 32, -1).mean(-1).abs() / stored.reshape(B, 32, -1).std(-1)
    assert float((ratio / R - 1).abs().max()) < 0.2, ratio           # the offset did reach the stored tensor
    want = F.conv2d(F.silu(F.group_norm(stored, 32, gamma.double(), beta.double(), NC.EPI_EPS)), wc.double(), None, padding=1)
    tag = f"{tile} {NC.DTN[dtype]} R={R} sigma={sigma}"
    _cmp(got.permute(0, 3, 1, 2), want, bound, f"consumer, producer's partials {tag}")
    _cmp(ref.permute(0, 3, 1, 2), want, bound, f"  consumer, statistics pass {tag}")
    _cmp(got, ref.cpu(), bound, f"  partials vs pass {tag}")
    _cmp_partials(ya._gn_part[0], ya, 32, bound, f"  {tag}")


@pytest.mark.parametrize("R,sigma", NC.epi_rungs(F32), ids=[_epi_ids(sg, R, R in NC.LADDER[F32]) for R, sg in NC.epi_rungs(F32)])
@pytest.mark.parametrize("mode", list(NC.EPI32))
def test_epilogue_partials_fp32_out(cuda, mode, R, sigma):
    """fp32-out producers of the split precision; the consumer normalises through rsvld_groupnorm_scale_shift_from_partials +
    rsvld_groupnorm_apply_split.  Bounds: the consumer convolution's (1e-4 of range, tests/test_gpu_split.py); the merged partials are
    GroupNorm statistics of the split precision: 2e-5."""
    from rsvld_amd import ops
    geo, label = NC.EPI32[mode]
    outputs = R in NC.LADDER[F32]
    c = NC.producer_case(geo, R, sigma, F16 if mode == "pair2" else F32, pre_norm=mode == "q8")
    gamma, beta, wc = c["gamma"], c["beta"], c["wc"]
    norm = (gamma.to(cuda), beta.to(cuda), NC.EPI_GROUPS, NC.EPI_EPS, True)
    pc, pcc = ops.pack_conv(c["w"], c["bias"], F32, cuda), ops.pack_conv(wc, None, F32, cuda)
    with ops.tuning(split_halo_min_wgs=0, halo_min_wgs=0, profiler=(prof := ops.LaunchProfiler())):
        if mode == "split3":
            with ops.f32_split(ops.ALL_SPLIT):
                ya = ops.conv2d(_nhwc(c["x"], cuda, F32), pc, pad=1, stats=True)
        elif mode == "pair2":
            with ops.f32_split(ops.ALL_SPLIT):
                ya = ops.conv2d(_nhwc(c["x"], cuda, F16), pc, pad=1, stats=True)
        else:
            n0 = (c["n0"][0].to(cuda), c["n0"][1].to(cuda), NC.EPI_GROUPS, NC.EPI_EPS, True)
            with ops.f32_split(ops.UNET_POLICY):
                ya = ops.conv2d(_nhwc(c["x"], cuda, F32), pc, pad=1, norm=n0, norm_group="conv1", stats=True)
        assert label in set(prof.summary()), set(prof.summary())
    assert ya.dtype == F32 and hasattr(ya, "_gn_part")
    tag = f"{mode} R={R} sigma={sigma}"
    _cmp_partials(ya._gn_part[0], ya, 32, NC.SPLIT_F32_OUT, f"producer {tag}", means=outputs)
    if not outputs:
        return
    with ops.f32_split(ops.ALL_SPLIT), ops.tuning(split_halo_min_wgs=0):
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            got = ops.conv2d(ya, pcc, pad=1, norm=norm)
        assert "groupnorm_ab_from_partials" in set(prof.summary())
        ref = ops.conv2d(ya.clone(), pcc, pad=1, norm=norm)
    stored = ya.double().cpu().permute(0, 3, 1, 2)
    ratio = stored.reshape(stored.shape[0], 32, -1).mean(-1).abs() / stored.reshape(stored.shape[0], 32, -1).std(-1)
    assert float((ratio / R - 1).abs().max()) < 0.2, ratio
    want = F.conv2d(F.silu(F.group_norm(stored, 32, gamma.double(), beta.double(), NC.EPI_EPS)), wc.double(), None, padding=1)
    _cmp(got.permute(0, 3, 1, 2), want, NC.SPLIT_CONV, f"  consumer, producer's partials {tag}")
    _cmp(ref.permute(0, 3, 1, 2), want, NC.SPLIT_CONV, f"  consumer, statistics pass {tag}")
    _cmp(got.permute(0, 3, 1, 2), ref.cpu().permute(0, 3, 1, 2), NC.SPLIT_CONV, f"  partials vs pass {tag}")


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: two-pass in registers already; these pin it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=NC.DTN.get)
@pytest.mark.parametrize("rows,C", NC.LN_SHAPES)
def test_layer_norm(cuda, rows, C, dtype):
    """rsvld_layernorm (16-bit), rsvld_layernorm_f32 and rsvld_layernorm_split (fp32 and planes out) on the ladder, and at the small
    spread on its top rung"""
    from rsvld_amd import ops
    for R, sigma in [(R, 1.0) for R in NC.LADDER[dtype]] + [(max(NC.LADDER[dtype]), NC.SMALL_SIGMA[0])]:
        c = NC.ln_case(rows, C, dtype, R, sigma)
        x, ga, be = c["x"].to(cuda, dtype), c["gamma"].to(cuda), c["beta"].to(cuda)
        tag = f"{rows}x{C} {NC.DTN[dtype]} R={R} sigma={sigma}"
        if dtype != F32:
            _cmp(ops.layer_norm(x, ga, be, c["eps"]), c["want"], NC.TOL16[dtype], f"layer_norm {tag}")
            continue
        _cmp(ops.layer_norm(x, ga, be, c["eps"]), c["want"], NC.F32_FAMILY, f"layer_norm_f32 {tag}")
        with ops.f32_split(ops.ALL_SPLIT):
            got = ops.layer_norm(x, ga, be, c["eps"])
            gp = ops.layer_norm(x, ga, be, c["eps"], planes=True)
        _cmp(got, c["want"], NC.SPLIT_LN_F32_OUT, f"  layer_norm split fp32 out {tag}")
        _cmp(gp.f32(), c["want"], NC.SPLIT_LN_PLANES_OUT, f"  layer_norm split planes out {tag}")
