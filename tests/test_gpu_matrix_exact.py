"""Every instantiation of dispatch_conv2 (csrc/conv_igemm.hip), dispatch_halo (csrc/conv_halo.hip) and the gemm256 forms on
EXACTLY COMPUTABLE operands: bit-for-bit parity with an fp64 reference, per instantiation.

The header says of the RSVLD_TUNE_* bits that "every combination computes the same function".  A tolerance cannot hold the code to
that cheaply: one pixel missing from a ragged tile, one K step dropped by the shorter of two K groups, moves a result by less than
the 16-bit parity bound.  Here the operands are small integers (fp16) or sparse ternary values (bf16), so every product, every
partial sum IN ANY ORDER, every epilogue step and the 16-bit store are exact: whatever the tile, ring depth, K split or staging,
the kernel must return the fp64 reference rounded once -- ``torch.equal``, no tolerance.

The conditions that make this true are properties of the INPUTS and are asserted by the builders on the CPU (also wherever the
suite runs without a GPU: tests/test_matrix_exact_cases.py walks the same tables):
  * t = conv + bias + rowvec, alpha * t and the final output survive a round trip through the output type;
  * the fp32 CPU product equals the fp64 one;
  * K * max|x| * max|w| in units of the operands' last bit stays below 2^24: no order of fp32 accumulation can round;
  * (halo statistics) every per-tile sum and sum of squares is an integer below 2^24.
Which instantiation a row lands in is arithmetic on its shape: the library's own planner (rsvld_plan_conv, a host-only query) is asked
about every row's descriptor and checked against the row's claim on the CPU, and the profiler label of ops.conv2d -- made from the same
plan -- is asserted on the GPU for every row, so a forced tile is proven to have run by name.

A tolerance case per instantiation (random normal operands as test_gpu_kernels.test_conv2d builds them, SiLU and GEGLU epilogues)
uses that module's ``_close`` unchanged."""
import functools
import math
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import GEMM_CASES, _close, _nhwc, _rt

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16]
_DTN = {F16: "fp16", BF16: "bf16"}

# rsvld_conv_desc.tune (include/rsvld_hip.h; tests/test_cabi.py pins rsvld_amd._lib to the header)
T256x64, T128x64, T128x128, T64x128 = 1, 2, 3, 4
ST2, ST3, ST4 = 2 << 3, 3 << 3, 4 << 3
NO_KSPLIT, REG, NW4, NW8, NO_GEMM256, ONE_TILE = 1 << 6, 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 12


# ============================================================================= the library's plan of a case
Inst = namedtuple("Inst", "bm bn stages ks staging")     # one instantiation of conv_igemm_kernel
_TENSOR = 1 << 12     # the plan queries compare a descriptor's pointers with NULL only: any other value stands for a tensor


def plan_conv(desc):
    """rsvld_plan_conv of an ``L.ConvDesc`` -> L.ConvPlan; the descriptor must be one rsvld_conv2d_nhwc accepts."""
    from rsvld_amd import _lib as L
    import ctypes
    plan = L.ConvPlan()
    rc = L.load().rsvld_plan_conv(ctypes.byref(desc), ctypes.byref(plan))
    assert rc == 0, L.ERRORS.get(rc, rc)
    return plan


def planned_inst(desc):
    """The implicit-GEMM instantiation the library plans for ``desc`` (gemm256 must not take it)."""
    p = plan_conv(desc)
    assert p.gemm256 == 0
    return Inst(p.bm, p.bn, p.stages, p.ks, "reg" if p.reg_staging else "lds")


def persistent_tiles(M, N, n_cu=256):
    """The tile enumeration of gemm256_kernel<PERSIST> (device code: nothing to query) -> (whole tiles, half tiles) of the launch."""
    nmt, nnt = (M + 255) // 256, (N + 255) // 256
    grid, ntiles, whole, halves = min(nmt * nnt, n_cu), nmt * nnt, 0, 0
    q, r = ntiles >> 3, ntiles & 7
    for xcd in range(8):
        qx, step = q + (1 if xcd < r else 0), (grid - xcd + 7) >> 3
        rem = qx % step
        if 0 < rem and 2 * rem <= step:
            whole, halves = whole + qx - rem, halves + 2 * rem
        else:
            whole += qx
    return whole, halves


# ============================================================================= shapes
# mode: "p1" stride 1, pad k // 2;  "s2" stride 2 with the VAE's asymmetric pad (0, 0, 1, 1);  "up" nearest x2 folded in, pad k // 2
Shape = namedtuple("Shape", "B H W C1 C2 Cout k mode")


def geometry(s):
    """-> (Ho, Wo, M, K chunks of 8 channels per segment) with ops._conv_geometry's arithmetic."""
    Hin, Win = (2 * s.H, 2 * s.W) if s.mode == "up" else (s.H, s.W)
    if s.mode == "s2":
        Ho, Wo = (Hin + 1 - s.k) // 2 + 1, (Win + 1 - s.k) // 2 + 1
    else:
        Ho, Wo = Hin + 2 * (s.k // 2) - s.k + 1, Win + 2 * (s.k // 2) - s.k + 1
    return Ho, Wo, s.B * Ho * Wo, s.k * s.k * (s.C1 + s.C2) // 8


def nk_of(s, seg=1):
    return (seg * geometry(s)[3] + 7) // 8


def conv_desc(s, tune, dtype=0, out_f32=0, cout_p=None):
    """The rsvld_conv_desc ops.conv2d builds for case shape ``s`` (``dtype`` / ``out_f32``: RSVLD_* operand form and output code), without
    tensors: for the plan queries.  A rowvec is set, as in every exact case."""
    from rsvld_amd import _lib as L
    Ho, Wo, _, _ = geometry(s)
    pad = 0 if s.mode == "s2" else s.k // 2
    return L.ConvDesc(x=_TENSOR, x2=_TENSOR if s.C2 else None, w=_TENSOR, rowvec=_TENSOR, out=_TENSOR, B=s.B, H=s.H, W=s.W, Cin=s.C1,
                      Cin2=s.C2, Cout=cout_p or s.Cout, KH=s.k, KW=s.k, stride=2 if s.mode == "s2" else 1, pad_t=pad, pad_l=pad, Ho=Ho,
                      Wo=Wo, upsample=int(s.mode == "up"), dtype=dtype, out_f32=out_f32, alpha=1.0, beta=1.0, tune=tune)


def linear_desc(M, K, N, tune):
    """ops.linear's descriptor of an [M, K] x [N, K] layer with a 16-bit output (no rowvec)."""
    from rsvld_amd import _lib as L
    return L.ConvDesc(x=_TENSOR, w=_TENSOR, out=_TENSOR, B=1, H=1, W=M, Cin=K, Cout=N, KH=1, KW=1, stride=1, Ho=1, Wo=M, alpha=1.0,
                      beta=1.0, tune=tune)


def conv_kwargs(s):
    return {"p1": dict(pad=s.k // 2), "s2": dict(stride=2, pad=(0, 0, 1, 1)), "up": dict(upsample=True, pad=s.k // 2)}[s.mode]


def shape_a(cout):
    """Exact case A: B = 3, 9 x 11 -> M = 297 = 256 + 41 = 2 * 128 + 41 = 4 * 64 + 41 (ragged last tile of every BM, more than one
    block); sources 72 | 48: the seam is no multiple of 64 channels; 3 x 3 x 120 = 135 eight-channel pieces = 16 K steps + 7 pieces:
    nk = 17, odd (the second of two K groups runs 8 steps, the first 9) with a partial last step."""
    return Shape(3, 9, 11, 72, 48, cout, 3, "p1")


def shape_b(cout, mode, k):
    """Exact case B, one source.  3 x 3: 120 channels (nk = 17 as in case A); 1 x 1: 1032 channels = 129 pieces (nk = 17, one piece in
    the last step).  "s2": 3 x 19 x 23 -> 9 x 11 (3 x 3, M = 297) / 10 x 12 (1 x 1, M = 360 = 256 + 104 = 5 * 64 + 40);
    "up": 3 x 5 x 6 -> 10 x 12 (M = 360)."""
    c = 120 if k == 3 else 1032
    return Shape(3, 19, 23, c, 0, cout, k, "s2") if mode == "s2" else Shape(3, 5, 6, c, 0, cout, k, "up")


# ============================================================================= the instantiation table
# One row per instantiation of conv_igemm.hip's launch table (both 16-bit types run every row).  ``label``: the profiler label of
# ops.conv2d names the tile family of the kernel that ran, forced tiles included; it is asserted for every row.
# ``b``: (mode, k) of exact case B, stride 2 and up-sampling alternating down the table; None: the row runs case A only.
Row = namedtuple("Row", "name tune cout inst label b a_shape")
L32, L64, L6464, L64128, L128 = ("conv_igemm_256x32", "conv_igemm_128x64", "conv_igemm_64x64", "conv_igemm_64x128", "conv_igemm_128x128")
L25664 = "conv_igemm_256x64"


def _row(name, tune, cout, inst, label, b, a_shape=None):
    return Row(name, tune, cout, Inst(*inst), label, b, a_shape or shape_a(cout))


ROWS = [
    # Cout 24 <= 32: 256x32 whatever the tune bits say
    _row("256x32", 0, 24, (256, 32, 2, 1, "lds"), L32, ("s2", 3)),
    _row("256x32_reg", REG, 24, (256, 32, 2, 1, "reg"), L32, ("up", 3)),
    # Cout 48 <= 64: tile mask 1 -> 256x64; otherwise 128x64 at the ring depth of the stage bits (2 = default; mask 2 names the default)
    _row("256x64", T256x64, 48, (256, 64, 2, 1, "lds"), L25664, ("s2", 3)),
    _row("256x64_reg", T256x64 | REG, 48, (256, 64, 2, 1, "reg"), L25664, ("up", 3)),
    _row("128x64", 0, 48, (128, 64, 2, 1, "lds"), L64, ("s2", 3)),
    _row("128x64_mask2", T128x64, 48, (128, 64, 2, 1, "lds"), L64, ("up", 3)),
    _row("128x64_st3", ST3, 48, (128, 64, 3, 1, "lds"), L64, ("s2", 3)),
    _row("128x64_st4", ST4, 48, (128, 64, 4, 1, "lds"), L64, ("up", 3)),
    _row("128x64_reg", REG, 48, (128, 64, 2, 1, "reg"), L64, ("s2", 3)),
    # Cout 176 > 64 (48 channels in the last column tile of BN 64 and of BN 128), M_plan <= 360: wg64x128 = ceil(M / 64) * 2 <= 12 < 256 -> 64x64; wg64 = ceil(M / 64) * 3 <= 18 <= 256 and nk = 17 >= 16
    # -> two K groups; NO_KSPLIT -> their one-group twin (case B of that row is a 1 x 1 kernel)
    _row("64x64_ks2", 0, 176, (64, 64, 4, 2, "lds"), L6464, ("up", 3)),
    _row("64x64", NO_KSPLIT, 176, (64, 64, 4, 1, "lds"), L6464, ("s2", 1)),
    # tile mask 4 -> 64x128: wg64x128 <= 256 and nk >= 16 -> two K groups; NO_KSPLIT or stage bits 3 -> 3 stages; 4 -> 4; 2 -> the double buffer
    _row("64x128_ks2", T64x128, 176, (64, 128, 3, 2, "lds"), L64128, ("up", 3)),
    _row("64x128_st3", T64x128 | NO_KSPLIT, 176, (64, 128, 3, 1, "lds"), L64128, ("s2", 3)),
    _row("64x128_st4", T64x128 | ST4, 176, (64, 128, 4, 1, "lds"), L64128, ("up", 3)),
    _row("64x128_st2", T64x128 | ST2, 176, (64, 128, 2, 1, "lds"), L64128, ("s2", 3)),
    _row("64x128_reg", T64x128 | REG, 176, (64, 128, 2, 1, "reg"), L64128, ("up", 3)),
    # tile mask 3 -> 128x128 (the 64x64 / 64x128 re-tiling of small grids is for mask 0 / 4 only); case B of the first row is 1 x 1
    _row("128x128", T128x128, 176, (128, 128, 2, 1, "lds"), L128, ("s2", 1)),
    _row("128x128_st3", T128x128 | ST3, 176, (128, 128, 3, 1, "lds"), L128, ("up", 3)),
    _row("128x128_st4", T128x128 | ST4, 176, (128, 128, 4, 1, "lds"), L128, ("s2", 3)),
    _row("128x128_reg", T128x128 | REG, 176, (128, 128, 2, 1, "reg"), L128, ("up", 3)),
    # the same three tiles reached by the DEFAULT routing (tune 0): routed by their grid alone.  Sources 24 | 16: 45 pieces, nk = 6.
    # 2 x 63 x 66 = 8316 rows: wg64x128 = 130 * 2 = 260 >= 256 (no 64x64, no K groups), wg128 = 65 * 2 = 130 < 256 -> 64x128, 3 stages
    _row("64x128_default", 0, 176, (64, 128, 3, 1, "lds"), L64128, None, Shape(2, 63, 66, 24, 16, 176, 3, "p1")),
    # 2 x 63 x 65 = 8190 rows, sources 72 | 48 (nk = 17): wg64x128 = 128 * 2 = 256 exactly -> 64x128 with two K groups
    _row("64x128_ks2_default", 0, 176, (64, 128, 3, 2, "lds"), L64128, None, Shape(2, 63, 65, 72, 48, 176, 3, "p1")),
    # 2 x 90 x 91 = 16380 rows: wg128 = 128 * 2 = 256 -> 128x128
    _row("128x128_default", 0, 176, (128, 128, 2, 1, "lds"), L128, None, Shape(2, 90, 91, 24, 16, 176, 3, "p1")),
]
SMALL_ROWS = [r for r in ROWS if r.b is not None]
# cross-instantiation equality on ONE call: every row of a Cout family runs case A on the same shape and operands
FAMILY_176 = [r for r in SMALL_ROWS if r.cout == 176]
FAMILY_48 = [r for r in SMALL_ROWS if r.cout == 48]

# Multi-segment instantiations (SEG = 3: RSVLD_SPLIT, bf16 planes x weight triples; SEG = 2: RSVLD_F16W2, fp16 x weight pairs, and
# RSVLD_F16W1, the pair kernels over ONE segment) exist for the LDS-DMA staging only: one row per tile family.
# nk = ceil(seg * 135 / 8) = 51 (triples), 34 (pairs); RSVLD_F16W1 is 1 x 1 over 1032 channels: nk = 17 -- all >= 16.
SegRow = namedtuple("SegRow", "name tune cout inst")
SEG_ROWS = [
    SegRow("256x32", 0, 24, Inst(256, 32, 2, 1, "lds")),
    SegRow("128x64", 0, 48, Inst(128, 64, 2, 1, "lds")),
    SegRow("64x64_ks2", 0, 176, Inst(64, 64, 4, 2, "lds")),
    SegRow("64x64", NO_KSPLIT, 176, Inst(64, 64, 4, 1, "lds")),
    SegRow("64x128_ks2", T64x128, 176, Inst(64, 128, 3, 2, "lds")),
    SegRow("64x128_st3", T64x128 | NO_KSPLIT, 176, Inst(64, 128, 3, 1, "lds")),
    SegRow("128x128", T128x128, 176, Inst(128, 128, 2, 1, "lds")),
]
SEG_MODES = {"split3": 3, "pair2": 2, "w1": 1}     # -> K segments per tap that the kernel walks
SEG_SIDES = ("xlo", "wlo")                          # which operand carries a non-zero low part


def seg_shape(mode, cout):
    return Shape(3, 9, 11, 1032, 0, cout, 1, "p1") if mode == "w1" else shape_a(cout)


# Halo kernel, sources 128 | 64, W = 45 (the second tile column holds 13 pixels), two heights: H = 19 is three rows of 8 x 32 tiles, the
# last one 3 pixels high -- of the 8-wave kernel's last 16-row tile the first 8-row sub-tile is partly filled and the second absent;
# H = 27 is four rows, the last one 3 pixels high -- there the second sub-tile is the partly filled one.
# Cout 44 (packed to 48) and 188 (packed to 192): the pad channels are part of every comparison, with their zeros.
HaloRow = namedtuple("HaloRow", "name tune cout inst label")
HALO_SHAPES = [(2, 19, 45, 128, 64), (1, 27, 45, 128, 64)]
HALO_ROWS = [
    HaloRow("bn64_nw4", NW4, 44, (64, 4), "conv_halo_64"),          # Cout <= 64: the 8 x 32 tile of conv_halo_kernel, four waves
    HaloRow("bn128_nw4", NW4, 188, (128, 4), "conv_halo_128"),      # (also the default here: at most 2 * 2 * 2 * 2 = 16 workgroups of 16 x 32 < 192)
    HaloRow("bn128_nw8", NW8, 188, (128, 8), "conv_halo_128"),      # forced
]

# gemm256: (M, K, N) of three GEMM_CASES rows, here with act none and a residual at alpha 0.5 / beta 2
GEMM_ROWS = [
    ("whole_tiles", GEMM_CASES[0][:3]),      # 17 x 15 = 255 tiles on 255 workgroups: 32 / 31 per XCD, no half-tile round
    ("half_tile_round", GEMM_CASES[11][:3]),  # (9216, 192, 2560): 360 tiles = 45 per XCD: one round + 13 tiles cut into 26 halves, on every XCD
    ("ragged_n_tile", GEMM_CASES[4][:3]),     # (4352, 256, 4104): a column tile of 8 channels
]


# ============================================================================= operand generators (CPU, deterministic)
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _sparse_ternary(g, shape, density):
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).double()


def exact_operands(g, dtype, xshape, wshape):
    """fp16: integers x in [-3, 3], w in [-2, 2].  bf16 (8 significant bits): x uniform over {-1, 0, 1}, w in {-1, 0, 1}, non-zero with
    probability 1/8."""
    if dtype == F16:
        return _ints(g, xshape, -3, 3), _ints(g, wshape, -2, 2)
    return _ints(g, xshape, -1, 1), _sparse_ternary(g, wshape, 1.0 / 8)


def _survives(t, dtype):
    return torch.equal(t.to(dtype).double(), t)


def _conv_ref(xcat, w, s):
    """The plain convolution of case shape ``s`` on NCHW tensors of any float type."""
    if s.mode == "up":
        xcat = F.interpolate(xcat, scale_factor=2, mode="nearest")
    if s.mode == "s2":
        return F.conv2d(F.pad(xcat, (0, 1, 0, 1)), w, None, stride=2)
    return F.conv2d(xcat, w, None, padding=s.k // 2)


def _check_exact(x, w, conv, s, dtype, out_dtype, t, alpha, out, unit=1.0):
    """The input-side conditions of an exact case (module docstring).  ``unit``: the operands' last bit; ``dtype`` None: the caller has
    checked that the operands fit their 16-bit parts."""
    assert dtype is None or (_survives(x, dtype) and _survives(w, dtype))
    K = s.k * s.k * (s.C1 + s.C2)
    assert K * float(x.abs().max()) * float(w.abs().max()) / unit < 2 ** 24, "an fp32 partial sum could round"
    assert torch.equal(_conv_ref(x.float(), w.float(), s).double(), conv), "fp32 and fp64 references differ"
    for name, v in (("t", t), ("alpha * t", alpha * t), ("out", out)):
        assert _survives(v, out_dtype), f"{name} is not representable in {out_dtype} (max {float(v.abs().max())})"


@functools.lru_cache(maxsize=None)
def build_conv_exact(dtype, s, epi, cout_p=None):
    """Exact case on shape ``s``.  ``epi``: "A" bias + rowvec (a column slice of a table twice as wide) + residual, alpha 0.5, beta 2;
    "B" bias + rowvec, no residual;  "H" as A with alpha = beta = 1 (the halo rows).  ``cout_p``: Cout packed to a multiple of 8, the
    rowvec / residual of the pad channels are zero.  Returns CPU tensors (NCHW operands in fp64; ``want``: NHWC fp64, cout_p wide);
    the cache hands the same objects to every test: they are read, never written."""
    g = _gen("conv", _DTN[dtype], tuple(s), epi)
    cp = cout_p or s.Cout
    x, w = exact_operands(g, dtype, (s.B, s.C1 + s.C2, s.H, s.W), (s.Cout, s.C1 + s.C2, s.k, s.k))
    Ho, Wo, _, _ = geometry(s)
    b = _ints(g, (s.Cout,), -4, 4)
    rv = torch.zeros(s.B, 2 * cp, dtype=torch.float64)
    rv[:, :s.Cout], rv[:, cp:cp + s.Cout] = _ints(g, (s.B, s.Cout), -4, 4), _ints(g, (s.B, s.Cout), -4, 4)
    res = None
    if epi in ("A", "H"):
        res = torch.zeros(s.B, Ho, Wo, cp, dtype=torch.float64)
        res[..., :s.Cout] = _ints(g, (s.B, Ho, Wo, s.Cout), -8, 8)
    alpha, beta = (0.5, 2.0) if epi == "A" else (1.0, 1.0)
    conv = _conv_ref(x, w, s)
    rv_used = rv[:, cp:] if epi in ("A", "H") else rv[:, :cp]
    t = F.pad((conv + b[None, :, None, None]).permute(0, 2, 3, 1), (0, cp - s.Cout)) + rv_used[:, None, None, :]
    want = alpha * t + (beta * res if res is not None else 0.0)
    _check_exact(x, w, conv, s, dtype, dtype, t, alpha, want)
    return dict(x=x, w=w, b=b, rv=rv, res=res, alpha=alpha, beta=beta, want=want, epi=epi, cp=cp)


def run_conv_exact(ops, dev, dtype, s, c, **extra):
    """The ops.conv2d call of an exact case ``c`` on ``dev`` -> NHWC output."""
    x = c["x"]
    pc = ops.pack_conv(c["w"], c["b"], dtype, dev, cin_split=(s.C1, s.C2) if s.C2 else None)
    rv = c["rv"].to(dev, F32)
    kw = dict(conv_kwargs(s), rowvec=rv[:, c["cp"]:] if c["epi"] in ("A", "H") else rv[:, :c["cp"]].contiguous(),
              alpha=c["alpha"], beta=c["beta"])
    if c["res"] is not None:
        kw["residual"] = c["res"].to(dev, dtype)
    if s.C2:
        kw["x2"] = _nhwc(x[:, s.C1:], dtype, dev)
    return ops.conv2d(_nhwc(x[:, :s.C1], dtype, dev), pc, **kw, **extra)


@functools.lru_cache(maxsize=None)
def build_f32_out_exact(dtype):
    """256x32 only: Cout 3 packed to 8 with an fp32 output (the networks' last convolution): bias, no residual."""
    s = Shape(3, 9, 11, 72, 0, 3, 3, "p1")
    g = _gen("f32out", _DTN[dtype])
    x, w = exact_operands(g, dtype, (s.B, s.C1, s.H, s.W), (s.Cout, s.C1, s.k, s.k))
    b = _ints(g, (s.Cout,), -4, 4)
    conv = _conv_ref(x, w, s)
    t = (conv + b[None, :, None, None]).permute(0, 2, 3, 1)
    _check_exact(x, w, conv, s, dtype, F32, t, 1.0, t)
    return dict(s=s, x=x, w=w, b=b, want=t)


@functools.lru_cache(maxsize=None)
def build_seg_exact(mode, side, cout):
    """Exact case A for a multi-segment kernel: operands whose LOW part is non-zero on one side at a time, so the dropped lo * lo term
    is zero and the fp64 reference is exact.  "xlo": activations a + b 2^-9 (a in [-3, 3], b in [-3, 3]: fp16 holds them whole, bf16
    planes as hi + lo) x integer weights in [-2, 2];  "wlo": integer activations in [-2, 2] x weights a + b 2^-12 (a in [-1, 1], b in
    [-3, 3]: an fp16 pair or a bf16 triple holds them as hi + lo; RSVLD_F16W1 ROUNDS its weights to fp16, so there b 2^-9).  Output and
    residual are fp32."""
    s = seg_shape(mode, cout)
    g = _gen("seg", mode, side, cout)
    xs, ws = (s.B, s.C1 + s.C2, s.H, s.W), (s.Cout, s.C1 + s.C2, s.k, s.k)
    if side == "xlo":
        x, w, unit = _ints(g, xs, -3, 3) + _ints(g, xs, -3, 3) * 2.0 ** -9, _ints(g, ws, -2, 2), 2.0 ** -9
    else:
        unit = 2.0 ** -9 if mode == "w1" else 2.0 ** -12
        x, w = _ints(g, xs, -2, 2), _ints(g, ws, -1, 1) + _ints(g, ws, -3, 3) * unit
    # the two 16-bit parts the packers / to_planes make hold each operand whole
    lo_dt = BF16 if mode == "split3" else F16
    for v, parts in ((x, 2 if mode == "split3" else 1), (w, 1 if mode == "w1" else 2)):
        hi = v.to(lo_dt).double()
        assert torch.equal(hi + ((v - hi).to(lo_dt).double() if parts == 2 else 0.0), v), "an operand does not fit its 16-bit parts"
    Ho, Wo, _, _ = geometry(s)
    b, rv = _ints(g, (s.Cout,), -4, 4), _ints(g, (s.B, 2 * s.Cout), -4, 4)
    res = _ints(g, (s.B, Ho, Wo, s.Cout), -8, 8)
    conv = _conv_ref(x, w, s)
    t = (conv + b[None, :, None, None]).permute(0, 2, 3, 1) + rv[:, None, None, s.Cout:]
    want = 0.5 * t + 2.0 * res
    _check_exact(x, w, conv, s, None, F32, t, 0.5, want, unit=unit)
    return dict(s=s, x=x, w=w, b=b, rv=rv, res=res, want=want)


def halo_partials(want, th=8, tw=32):
    """Per-(image, 8 x 32 tile, channel) (sum, sum of squares) of an NHWC fp64 tensor -> [B, tiles, C, 2], tiles row-major."""
    B, H, W, C = want.shape
    ty, tx = (H + th - 1) // th, (W + tw - 1) // tw
    p = F.pad(want, (0, 0, 0, tx * tw - W, 0, ty * th - H)).reshape(B, ty, th, tx, tw, C)
    return torch.stack([p.sum((2, 4)), (p * p).sum((2, 4))], -1).reshape(B, ty * tx, C, 2)


@functools.lru_cache(maxsize=None)
def build_halo_exact(dtype, cout, hs):
    B, H, W, C1, C2 = hs
    cp = (cout + 7) // 8 * 8
    c = build_conv_exact(dtype, Shape(B, H, W, C1, C2, cout, 3, "p1"), "H", cout_p=cp)
    part = halo_partials(c["want"])
    assert float(part.abs().max()) < 2 ** 24 and torch.equal(part, part.round()), "a tile sum is no integer below 2^24"
    assert torch.equal(c["want"][..., cout:], torch.zeros_like(c["want"][..., cout:]))
    return dict(c, part=part)


@functools.lru_cache(maxsize=None)
def build_gemm_operands(dtype, M, K, N):
    g = _gen("gemm", _DTN[dtype], M, K, N)
    x, w = exact_operands(g, dtype, (M, K), (N, K))
    return dict(x=x.float(), w=w.float(), b=_ints(g, (N,), -4, 4).float(), res=_ints(g, (M, N), -8, 8).float())


def gemm_reference(dtype, o, rows=None):
    """fp64 reference of out = 0.5 (x W^T + b) + 2 res on the first ``rows`` rows, with the input-side conditions asserted."""
    x, res = (o["x"], o["res"]) if rows is None else (o["x"][:rows], o["res"][:rows])
    assert _survives(o["x"].double(), dtype) and _survives(o["w"].double(), dtype)
    assert o["x"].shape[1] * float(o["x"].abs().max()) * float(o["w"].abs().max()) < 2 ** 24
    prod = x.double() @ o["w"].double().t()
    assert torch.equal((x @ o["w"].t()).double(), prod), "fp32 and fp64 references differ"
    t = prod + o["b"].double()
    want = 0.5 * t + 2.0 * res.double()
    for name, v in (("t", t), ("alpha * t", 0.5 * t), ("out", want)):     # alpha * t: gemm256 rounds it to 16 bits before the residual add
        assert _survives(v, dtype), f"{name} is not representable in {dtype}"
    return want


@functools.lru_cache(maxsize=None)
def build_gemm_exact(dtype, M, K, N):
    o = build_gemm_operands(dtype, M, K, N)
    return dict(o, want=gemm_reference(dtype, o))


@functools.lru_cache(maxsize=None)
def build_conv_random(dtype, s, geglu):
    """Random normal operands exactly as test_gpu_kernels.test_conv2d builds them; SiLU or GEGLU on top."""
    g = _gen("rand", _DTN[dtype], tuple(s), geglu)
    Cin = s.C1 + s.C2
    x = _rt(torch.randn(s.B, Cin, s.H, s.W, generator=g), dtype)
    w = _rt(torch.randn(s.Cout, Cin, s.k, s.k, generator=g) / math.sqrt(Cin * s.k * s.k), dtype)
    b = torch.randn(s.Cout, generator=g) * 0.1
    y = _conv_ref(x, w, s) + b[None, :, None, None]
    if geglu:
        val, gate = y.chunk(2, dim=1)
        want = val * F.gelu(gate)
    else:
        want = F.silu(y)
    return dict(x=x, w=w, b=b, want=want)


# ============================================================================= the GPU tests
class _Names:
    """On the hook of ops.LaunchProfiler: the launch labels, no events (as tests/guarded.LaunchRecorder)."""

    def __init__(self):
        self.names = []

    def run(self, name, flops, nbytes, fn):
        self.names.append(name)
        return fn()


def _ids(rows):
    return [r.name for r in rows]


def _run_row(ops, dev, dtype, row, s, c, **extra):
    rec = _Names()
    with ops.tuning(tune=row.tune, use_halo=False, profiler=rec):
        got = run_conv_exact(ops, dev, dtype, s, c, **extra)
    assert rec.names == [row.label], f"{row.name} ran {rec.names}"
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_conv_exact_case_a(cuda, dtype, row):
    """Two sources with a seam inside a K step, ragged M / Cout / K, bias + strided rowvec + residual at alpha 0.5, beta 2."""
    from rsvld_amd import ops
    c = build_conv_exact(dtype, row.a_shape, "A")
    got = _run_row(ops, cuda, dtype, row, row.a_shape, c)
    assert torch.equal(got.cpu(), c["want"].to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("row", SMALL_ROWS, ids=_ids(SMALL_ROWS))
def test_conv_exact_case_b(cuda, dtype, row):
    """One source, no residual: stride 2 under the asymmetric pad, or the folded nearest x2; 3 x 3 or 1 x 1."""
    from rsvld_amd import ops
    s = shape_b(row.cout, *row.b)
    c = build_conv_exact(dtype, s, "B")
    got = _run_row(ops, cuda, dtype, row, s, c)
    assert torch.equal(got.cpu(), c["want"].to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("row", SMALL_ROWS, ids=_ids(SMALL_ROWS))
def test_conv_tolerance_silu_geglu(cuda, dtype, row):
    """Random normal operands through the same instantiation, SiLU and GEGLU epilogues, against torch fp32 at the parity tolerance."""
    from rsvld_amd import ops, _lib as L
    for geglu in (False, True):
        cout = 32 if (geglu and row.cout == 24) else row.cout        # GEGLU pairs need Cout % 16 == 0; 32 stays on 256x32
        s = shape_a(cout)._replace(C1=120, C2=0)
        c = build_conv_random(dtype, s, geglu)
        rec = _Names()
        with ops.tuning(tune=row.tune, use_halo=False, profiler=rec):
            got = ops.conv2d(_nhwc(c["x"], dtype, cuda), ops.pack_conv(c["w"], c["b"], dtype, cuda, geglu=geglu), pad=1,
                             act=L.ACT_GEGLU if geglu else L.ACT_SILU)
        assert rec.names == [row.label], rec.names
        assert got.shape[-1] == (cout // 2 if geglu else cout)
        _close(got.permute(0, 3, 1, 2), c["want"], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("tune", [0, REG], ids=["lds", "reg"])
def test_conv_256x32_f32_out_pad_channels_are_zero(cuda, dtype, tune):
    from rsvld_amd import ops
    c = build_f32_out_exact(dtype)
    rec = _Names()
    with ops.tuning(tune=tune, use_halo=False, profiler=rec):
        got = ops.conv2d(_nhwc(c["x"], dtype, cuda), ops.pack_conv(c["w"], c["b"], dtype, cuda), pad=1, out_f32=True)
    assert rec.names == [L32]
    assert got.dtype == F32 and got.shape[-1] == 8
    assert torch.equal(got[..., :3].cpu().double(), c["want"])
    assert torch.equal(got[..., 3:].cpu(), torch.zeros(got.shape[:3] + (5,)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("family", [FAMILY_176, FAMILY_48], ids=["cout176", "cout48"])
def test_conv_instantiations_return_the_same_tensor(cuda, dtype, family):
    """ONE call (case A), every instantiation that accepts it: tiles, ring depths, one or two K groups, both stagings -- equal outputs."""
    from rsvld_amd import ops
    s = shape_a(family[0].cout)
    c = build_conv_exact(dtype, s, "A")
    outs = {row.name: _run_row(ops, cuda, dtype, row, s, c) for row in family}
    first = outs[family[0].name]
    for name, o in outs.items():
        assert torch.equal(o, first), f"{name} differs from {family[0].name}"
    assert torch.equal(first.cpu(), c["want"].to(dtype))


def _seg_call(ops, dev, mode, c):
    s = c["s"]
    pc = ops.pack_conv(c["w"], c["b"], F32, dev, cin_split=(s.C1, s.C2) if s.C2 else None)
    adt = F32 if mode == "split3" else F16
    rv = c["rv"].to(dev, F32)
    kw = dict(pad=s.k // 2, rowvec=rv[:, s.Cout:], residual=c["res"].to(dev, F32), alpha=0.5, beta=2.0)
    if s.C2:
        kw["x2"] = _nhwc(c["x"][:, s.C1:], adt, dev)
    if mode == "w1":
        kw["group"] = "ff_out"
    policy = {"split3": ops.ALL_SPLIT, "pair2": ops.SplitPolicy(f16_weights=()), "w1": ops.UNET_POLICY}[mode]
    with ops.f32_split(policy):
        return ops.conv2d(_nhwc(c["x"][:, :s.C1], adt, dev), pc, **kw)


@pytest.mark.parametrize("side", SEG_SIDES)
@pytest.mark.parametrize("mode", list(SEG_MODES))
@pytest.mark.parametrize("row", SEG_ROWS, ids=_ids(SEG_ROWS))
def test_conv_multi_segment_exact(cuda, row, mode, side):
    """SEG = 3 (weight triples over planes), SEG = 2 (weight pairs) and RSVLD_F16W1 on every LDS-DMA tile family: the wrap of the
    channel index into the second / third segment, with the seam of two sources inside a K step."""
    from rsvld_amd import ops
    c = build_seg_exact(mode, side, row.cout)
    rec = _Names()
    with ops.tuning(tune=row.tune, use_halo=False, profiler=rec):
        got = _seg_call(ops, cuda, mode, c)
    label = [n for n in rec.names if n.startswith("conv_igemm")]
    tile = f"conv_igemm_{row.inst.bm}x{row.inst.bn}"       # (the split path's label names no tile)
    assert label == [{"split3": "conv_igemm_split", "pair2": tile + "_w2", "w1": tile + "_w1"}[mode]], rec.names
    assert got.dtype == F32
    assert torch.equal(got.cpu().double(), c["want"])


def _halo_call(ops, dev, dtype, row, c, hs):
    B, H, W, C1, C2 = hs
    rec = _Names()
    with ops.tuning(halo_min_wgs=0, tune=row.tune, profiler=rec):
        got = run_conv_exact(ops, dev, dtype, Shape(B, H, W, C1, C2, row.cout, 3, "p1"), c, stats=True)
    assert rec.names == [row.label], rec.names
    assert hasattr(got, "_gn_part")
    return got, got._gn_part[0]


_HS = dict(argvalues=HALO_SHAPES, ids=["h19", "h27"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("hs", **_HS)
@pytest.mark.parametrize("row", HALO_ROWS, ids=_ids(HALO_ROWS))
def test_halo_exact_output_and_partials(cuda, dtype, row, hs):
    """The halo kernels without a fused norm: the output AND the per-tile (sum, sum of squares) partials of the epilogue, bit for bit,
    ragged last tile row and column and the pad channels included."""
    from rsvld_amd import ops
    c = build_halo_exact(dtype, row.cout, hs)
    got, part = _halo_call(ops, cuda, dtype, row, c, hs)
    assert torch.equal(got.cpu(), c["want"].to(dtype))
    assert part.dtype == torch.float64 and tuple(part.shape) == tuple(c["part"].shape)
    assert torch.equal(part.cpu().double(), c["part"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("hs", **_HS)
def test_halo_8_wave_equals_4_wave(cuda, dtype, hs):
    from rsvld_amd import ops
    c = build_halo_exact(dtype, 188, hs)
    got4, part4 = _halo_call(ops, cuda, dtype, HALO_ROWS[1], c, hs)
    got8, part8 = _halo_call(ops, cuda, dtype, HALO_ROWS[2], c, hs)
    assert torch.equal(got4, got8) and torch.equal(part4, part8)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("case", GEMM_ROWS, ids=[n for n, _ in GEMM_ROWS])
def test_gemm256_exact_all_forms_and_implicit_gemm(cuda, dtype, case):
    """gemm256's persistent and one-tile forms and the implicit-GEMM kernel on the same Linear (RSVLD_TUNE_NO_GEMM256): equal to the
    fp64 reference and to each other.  With a residual gemm256 rounds alpha * t to 16 bits before the add; alpha * t is representable
    here (asserted by the builder), so that rounding is exact too."""
    from rsvld_amd import ops
    M, K, N = case[1]
    c = build_gemm_exact(dtype, M, K, N)
    x, res = c["x"].to(cuda, dtype), c["res"].to(cuda, dtype)
    pc = ops.pack_conv(c["w"], c["b"], dtype, cuda)
    outs = {}
    for name, tune, label in (("persistent", 0, "gemm_256x256"), ("one_tile", ONE_TILE, "gemm_256x256"), ("implicit_gemm", NO_GEMM256, L128)):
        rec = _Names()
        with ops.tuning(tune=tune, profiler=rec):
            outs[name] = ops.linear(x, pc, residual=res, alpha=0.5, beta=2.0)
        assert rec.names == [label], rec.names
    want = c["want"].to(dtype)
    for name, o in outs.items():
        assert torch.equal(o.cpu(), want), name
    assert torch.equal(outs["persistent"], outs["one_tile"]) and torch.equal(outs["persistent"], outs["implicit_gemm"])
