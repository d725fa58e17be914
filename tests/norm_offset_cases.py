"""Offset-dominated inputs for the normalisation kernels: the case generator, the fp64 references, the bounds and the CPU
emulations behind tests/test_gpu_norm_offset.py (walked without a GPU by tests/test_norm_offset_cases.py).

Why: a GroupNorm that forms its variance as E[x^2] - mean^2 from (sum, sum of squares) keeps it to 2^-p (mean / sigma)^2 relative
when the pair is held in a p-bit significand.  Inputs of the shape ``randn * a + b`` with |b| / a <= 0.25 -- every other
normalisation input of this suite -- cannot tell an fp32 pair from an fp64 one.  These can: each group sits at ``+-R sigma``.

Generator: ``x[b, g] = sigma randn + sign_g R sigma`` (random sign per group; LayerNorm: per row), rounded through the storage
type so that the fp64 reference and the kernel see the same values; gamma, beta ~ randn; fixed seeds.
Ladder: the top rung of a storage type is where it still resolves sigma into 16 steps, R <= 2^(p - 4) for a p-bit significand;
fp32 stops far below that, at the rung where an IDEAL fp32 affine still meets half the fp32 bounds (the fairness condition).
Reference: F.group_norm / F.layer_norm of ``x.double()``, (mean, biased variance) per group in fp64."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTN = {F16: "f16", BF16: "bf16", F32: "f32"}
SIGNIFICAND = {F16: 11, BF16: 8, F32: 24}

# mean / sigma per storage type: output checks, and (fp32) the rung where only the statistics are checked
LADDER = {F16: (8, 32, 128), BF16: (4, 16), F32: (8, 64)}
VAR_ONLY = {F16: (), BF16: (), F32: (512,)}

# ---------------------------------------------------------------------------------------------------------------------------------
# bounds, of the tensor's range: the ones the routes' own tests assert (tests/test_gpu_kernels.py _tol, tests/test_gpu_split.py
# test_group_norm_split / test_layer_norm_split, tests/test_gpu_f32.py REL), restated here so that the CPU checks need no GPU module
# ---------------------------------------------------------------------------------------------------------------------------------
TOL16 = {F16: 4e-3, BF16: 3e-2}          # _tol of test_gpu_kernels.py
SPLIT_F32_OUT, SPLIT_PLANES_OUT = 2e-5, 3e-5
SPLIT_LN_F32_OUT, SPLIT_LN_PLANES_OUT = 1e-5, 2e-5
F32_FAMILY = 2e-5                        # REL of test_gpu_f32.py
SPLIT_CONV = 1e-4                        # REL of test_gpu_split.py (the consumer convolution under the split precision)


def gn_bound(dtype, out="same"):
    """Output bound of a GroupNorm route: ``dtype`` = the storage type of its input, ``out`` in same / f32 / planes / family."""
    if dtype != F32:
        return TOL16[dtype]
    return {"f32": SPLIT_F32_OUT, "planes": SPLIT_PLANES_OUT, "family": F32_FAMILY}[out]


# ---------------------------------------------------------------------------------------------------------------------------------
# routes: the library's own answer (rsvld_plan_groupnorm, a host-only query: needs the built library, no device)
# ---------------------------------------------------------------------------------------------------------------------------------
def gn_plan(dtype, B, HW, C1, C2, groups):
    """-> rsvld_groupnorm_plan: ``small`` (the one-workgroup route), ``nchunks`` x ``rows_per_chunk`` of the partials route and the
    ``rows_in_flight`` of its statistics kernel."""
    import ctypes
    from rsvld_amd import _lib as L
    plan = L.GroupnormPlan()
    rc = L.load().rsvld_plan_groupnorm({F16: L.F16, BF16: L.BF16, F32: L.F32}[dtype], B, HW, C1, C2, groups, ctypes.byref(plan))
    assert rc == 0, L.ERRORS.get(rc, rc)
    return plan


def gn_route(dtype, HW, C1, C2, groups, B=1):
    """The statistics route of rsvld_groupnorm_nhwc / _scale_shift: the one-workgroup kernel (16-bit only) or the row-chunk partials."""
    return "small" if gn_plan(dtype, B, HW, C1, C2, groups).small else "partial"


GnShape = namedtuple("GnShape", "name B C1 C2 H W groups route16 why")
GN_SHAPES = [
    GnShape("small", 2, 256, 0, 19, 23, 32, "small", "one workgroup per (image, group): 437 rows of one 8-channel vector"),
    GnShape("gs2", 2, 64, 0, 48, 48, 32, "partial", "groups of 2 channels: four groups inside one 8-channel vector, 36 chunks of 64 rows"),
    GnShape("straddle", 1, 128, 64, 9, 33, 32, "partial", "two sources, groups of 6 channels: group 21 straddles them; 5 chunks, the last 41 rows"),
    GnShape("chunk512", 1, 32, 0, 512, 512, 8, "partial", "512 chunks of 512 rows: the longest fp32 runs inside a thread"),
]
F32_FAMILY_SHAPE = GnShape("family", 1, 64, 0, 48, 48, 32, "partial", "csrc/f32.hip: fp64 partial sums")
# fp32 input only: sums + pivots of 5 504 channels need 66 048 B of LDS, above the 64 KiB a kernel gets unasked
WIDE_SHAPE = GnShape("wide", 1, 5504, 0, 5, 7, 32, "partial", "C > 5 460: the statistics pass asks for more dynamic LDS")
GN_BY_NAME = {s.name: s for s in GN_SHAPES + [F32_FAMILY_SHAPE, WIDE_SHAPE]}
LN_SHAPES = [(77, 320), (50, 2048)]

# (sigma, eps): unit spread, and one small-spread case per route where eps is a visible part of var + eps
UNIT, SMALL_SIGMA = (1.0, 1e-6), (0.05, 1e-5)


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31 - 1)


def _group_var(x64, groups):
    B = x64.shape[0]
    xg = x64.reshape(B, groups, -1)
    return xg.mean(-1), xg.var(-1, unbiased=False)


@functools.lru_cache(maxsize=8)
def gn_case(name, dtype, R, sigma=1.0, eps=1e-6):
    """-> dict(x [B, C, H, W] fp32 holding values of ``dtype``, gamma, beta, want (fp64 GroupNorm), mean, var [B, groups] fp64, ...)"""
    s = GN_BY_NAME[name]
    C = s.C1 + s.C2
    g = torch.Generator().manual_seed(_seed(C, s.H, s.W, R, SIGNIFICAND[dtype], round(sigma * 100)))
    sign = torch.randint(0, 2, (s.B, s.groups), generator=g).float() * 2 - 1
    x = torch.randn(s.B, s.groups, C // s.groups, s.H, s.W, generator=g) * sigma + (sign * (R * sigma))[:, :, None, None, None]
    x = x.reshape(s.B, C, s.H, s.W).to(dtype).float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = F.group_norm(x.double(), s.groups, gamma.double(), beta.double(), eps)
    mean, var = _group_var(x.double(), s.groups)
    return dict(s=s, x=x, gamma=gamma, beta=beta, want=want, mean=mean, var=var, eps=eps, sigma=sigma, R=R, dtype=dtype)


@functools.lru_cache(maxsize=8)
def ln_case(rows, C, dtype, R, sigma=1.0, eps=1e-5):
    g = torch.Generator().manual_seed(_seed(rows, C, R, SIGNIFICAND[dtype], round(sigma * 100)))
    sign = torch.randint(0, 2, (rows, 1), generator=g).float() * 2 - 1
    x = (torch.randn(rows, C, generator=g) * sigma + sign * (R * sigma)).to(dtype).float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps)
    return dict(x=x, gamma=gamma, beta=beta, want=want, eps=eps, R=R, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# emulations (CPU, torch fp32 arithmetic = one rounding per operation)
# ---------------------------------------------------------------------------------------------------------------------------------
def round_out(y32, out):
    """The output rounding of a route: a 16-bit type, fp32 (none) or bf16 planes (hi = bf16(v), lo = bf16(v - hi))."""
    if out == "planes":
        hi = y32.bfloat16().float()
        return hi + (y32 - hi).bfloat16().float()
    if out in (F16, BF16):
        return y32.to(out).float()
    return y32


def affine_from_stats(x, mean, var, gamma, beta, groups, eps):
    """The kernels' affine from fp32 (mean, var) rows [B, groups]: a = gamma rstd, s = beta - mean a, y = a x + s, all fp32."""
    B, C = x.shape[:2]
    gs = C // groups
    rstd = 1.0 / torch.sqrt(var.float() + torch.tensor(eps, dtype=F32))
    a = gamma.float()[None, :] * rstd.repeat_interleave(gs, 1)
    sh = beta.float()[None, :] - mean.float().repeat_interleave(gs, 1) * a
    return a[:, :, None, None] * x.float() + sh[:, :, None, None]


def rel_err(got, want):
    want = want.double()
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def ideal_gn_error(c, out):
    """Fairness: ideal statistics (fp64, rounded to fp32) through the kernels' fp32 affine and output rounding, of the range."""
    y = affine_from_stats(c["x"], c["mean"], c["var"], c["gamma"], c["beta"], c["s"].groups, c["eps"])
    return rel_err(round_out(y, out), c["want"])


def ideal_gn_error_of(x, gamma, beta, groups, eps, out):
    """The same for any NCHW tensor (the stored output of a producer convolution)."""
    mean, var = _group_var(x.double(), groups)
    want = F.group_norm(x.double(), groups, gamma.double(), beta.double(), eps)
    return rel_err(round_out(affine_from_stats(x, mean, var, gamma, beta, groups, eps), out), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue partials: a producer 3x3 convolution whose output has spread sigma (its weights are scaled for it) and sits at +-R sigma
# per group of the consumer's GroupNorm (its bias), and the consumer's GroupNorm affine and 3x3 weights
# ---------------------------------------------------------------------------------------------------------------------------------
EPI16 = {"4wave": (2, 64, 128, 19, 40), "8wave": (2, 64, 512, 96, 128)}
EPI32 = {
    # mode: (B, Cin, Cout, H, W), the producer's label
    "split3": ((2, 64, 128, 19, 40), "conv_halo_128_split"),       # RSVLD_SPLIT: fp32 in (planes), weight triples
    "pair2": ((2, 64, 128, 19, 40), "conv_halo_128_w2"),           # RSVLD_F16W2: fp16 in, weight pairs, fp32 out
    "q8": ((1, 128, 128, 19, 37), "conv_halo_128_q8"),             # RSVLD_F16Q8: behind its own GroupNorm, e4m3 cross terms, fp32 out
}
EPI_GROUPS, EPI_EPS = 32, 1e-5


def epi_rungs(dtype):
    """(R, sigma) of the epilogue tests: the ladder at unit spread, the top rung at the small spread, (fp32) the statistics-only rung"""
    return [(R, 1.0) for R in LADDER[dtype]] + [(max(LADDER[dtype]), SMALL_SIGMA[0])] + [(R, 1.0) for R in VAR_ONLY[dtype]]


@functools.lru_cache(maxsize=4)
def producer_case(geo, R, sigma, dtype, pre_norm=False):
    """``dtype``: the storage type of the producer's operands (F32: none).  ``pre_norm``: the producer has a GroupNorm + SiLU of its
    own in front (the q8 form); its weights are then scaled by the measured spread of the un-biased output.
    -> dict(x, w, bias, gamma, beta, wc, n0 (the producer's own norm or None), stored (the producer's output on the CPU, fp32))"""
    B, Cin, Cout, H, W = geo
    g = torch.Generator().manual_seed(_seed(Cin, Cout, H, W, R, SIGNIFICAND[dtype], round(sigma * 100)))
    rt = (lambda t: t) if dtype == F32 else (lambda t: t.to(dtype).float())
    x = rt(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    sign = torch.randint(0, 2, (EPI_GROUPS,), generator=g).float() * 2 - 1
    bias = (sign * (R * sigma)).repeat_interleave(Cout // EPI_GROUPS)
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    wc = rt(torch.randn(8, Cout, 3, 3, generator=g) / (9 * Cout) ** 0.5)
    n0, xin = None, x
    if pre_norm:
        n0 = (1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g))
        xin = F.silu(F.group_norm(x, EPI_GROUPS, n0[0], n0[1], EPI_EPS))
        w = w / float(F.conv2d(xin, w, None, padding=1).std())
    w = rt(w * sigma)
    stored = rt(F.conv2d(xin, w, bias, padding=1))
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, wc=wc, n0=n0, stored=stored, R=R, sigma=sigma)


def ideal_ln_error(c, out):
    """The LayerNorm kernels' form with ideal statistics: ((x - mean) rstd) gamma + beta in fp32."""
    x64 = c["x"].double()
    mean = x64.mean(-1, keepdim=True).float()
    var = x64.var(-1, unbiased=False, keepdim=True).float()
    rstd = 1.0 / torch.sqrt(var + torch.tensor(c["eps"], dtype=F32))
    y = (c["x"] - mean) * rstd * c["gamma"][None, :] + c["beta"][None, :]
    return rel_err(round_out(y, out), c["want"])


def _rows_nhwc(c):
    s = c["s"]
    return c["x"].permute(0, 2, 3, 1).reshape(s.B, s.H * s.W, s.C1 + s.C2)


def _chunk_thread_terms(c):
    """gn_partial_kernel's geometry for ONE source: rows [B, nchunks, rows_per_chunk, C] (zero-padded, with the mask), the rows in
    flight ``rif`` and the order in which a thread meets its rows."""
    s = c["s"]
    assert s.C2 == 0
    C, HW = s.C1, s.H * s.W
    plan = gn_plan(c["dtype"], s.B, HW, C, 0, s.groups)
    nch, rpc, rif = plan.nchunks, plan.rows_per_chunk, plan.rows_in_flight
    xr = _rows_nhwc(c)
    pad = nch * rpc - HW
    xr = F.pad(xr, (0, 0, 0, pad))
    mask = F.pad(torch.ones(HW), (0, pad)).reshape(1, nch, rpc, 1)
    return xr.reshape(s.B, nch, rpc, C), mask, rif, rpc


def emulate_partial_sums_fp32(c):
    """The arithmetic this file was written against: per thread s += f, ss += f * f in fp32 over its rows (rsub, rsub + rif, ...),
    the rows-in-flight x group-size values added in fp32 (row outer, channel inner), the chunk partials merged in fp64;
    var = E[x^2] - mean^2.  -> (mean, var) fp64 [B, groups]."""
    s = c["s"]
    x, mask, rif, rpc = _chunk_thread_terms(c)
    B, nch, _, C = x.shape
    ts = torch.zeros(B, nch, rif, C)
    tq = torch.zeros(B, nch, rif, C)
    for r0 in range(0, rpc, rif):                      # a thread's rows, in order
        f = x[:, :, r0:r0 + rif]
        m = mask[:, :, r0:r0 + rif]
        n = f.shape[2]
        ts[:, :, :n] = ts[:, :, :n] + f * m
        tq[:, :, :n] = tq[:, :, :n] + (f * f) * m
    gs = C // s.groups
    gsum = torch.zeros(B, nch, s.groups)
    gsq = torch.zeros(B, nch, s.groups)
    for r in range(rif):
        for e in range(gs):
            gsum = gsum + ts[:, :, r, e::gs]
            gsq = gsq + tq[:, :, r, e::gs]
    n = float(s.H * s.W * gs)
    mean = gsum.double().sum(1) / n
    var = (gsq.double().sum(1) / n - mean * mean).clamp_min(0.0)
    return mean, var


def emulate_partial_sums_pivot(c):
    """The pivoted form: k = the channel's value in the chunk's first row; per thread s += (f - k), q += (f - k)^2 in fp32, the rows in
    flight added per channel in fp32; from there fp64: (sum, sumsq) = (s + n k, q + k (2 s + n k)), groups, chunks."""
    s = c["s"]
    x, mask, rif, rpc = _chunk_thread_terms(c)
    B, nch, _, C = x.shape
    k = x[:, :, :1]
    ts = torch.zeros(B, nch, rif, C)
    tq = torch.zeros(B, nch, rif, C)
    for r0 in range(0, rpc, rif):
        d = (x[:, :, r0:r0 + rif] - k) * mask[:, :, r0:r0 + rif]
        n = d.shape[2]
        ts[:, :, :n] = ts[:, :, :n] + d
        tq[:, :, :n] = tq[:, :, :n] + d * d
    cs, cq = torch.zeros(B, nch, C), torch.zeros(B, nch, C)
    for r in range(rif):                               # the rows in flight, still fp32
        cs, cq = cs + ts[:, :, r], cq + tq[:, :, r]
    cs, cq = cs.double(), cq.double()
    nrows = mask.double().sum(2)                       # [1, nch, 1]
    kd = k[:, :, 0].double()
    csum = cs + nrows * kd
    csq = cq + kd * (2.0 * cs + nrows * kd)
    gs = C // s.groups
    n = float(s.H * s.W * gs)
    mean = csum.reshape(B, nch, s.groups, gs).sum((1, 3)) / n
    var = (csq.reshape(B, nch, s.groups, gs).sum((1, 3)) / n - mean * mean).clamp_min(0.0)
    return mean, var


def stats_errors(mean, var, c):
    """-> (max |mean - ref| / sigma, max relative variance error) over (image, group)"""
    em = float((mean.double() - c["mean"]).abs().max()) / c["sigma"]
    ev = float(((var.double() - c["var"]).abs() / c["var"]).max())
    return em, ev
