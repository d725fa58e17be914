"""Every kernel behind ops.py on poisoned, guard-banded buffers (tests/guarded.py).

The kernel sources promise things about memory OUTSIDE an operand -- "rows past the end re-read a valid address (never stored)",
"rows past Nk re-read the last key and are masked in the softmax", "clamped rows carry P = 0", "zero-fill by predicate", "a position
outside the cache is clamped, never written past it" -- and the parity tests cannot see a broken promise: their tensors come from
torch's caching allocator, where the neighbour is slack or a dead tensor of finite numbers.  Here every operand, output and workspace
of a call lies between guards of 0xFF bytes (NaN in every float type), flush against the rear guard, and after the call

  1. every guard is intact,  2. every operand is bit-identical to what was placed (documented in-place updates excepted),
  3. every returned element is finite (written, and free of poison),  4. the result equals the same call on ordinary tensors, bit for bit.

The VALUES are tied to the fp32 / fp64 references by the parity tests whose shape tables are imported here; each case's comment says
which clamp or predicate it leans on.  No case provokes a fault: a stray access of a guarded run lands in memory the test owns.
``declared_wrappers()`` feeds the census of tests/test_guarded_instrument.py: a public wrapper of ops.py without a case fails it."""
import contextlib
import math

import pytest
import torch

import guarded as G
from test_gpu_kernels import CONV_CASES, GEMM_CASES, GN_CASES, HALO_CASES, attn_plan
from test_gpu_matrix_exact import linear_desc, plan_conv
from test_gpu_split import CONV_CASES as SPLIT_CONV_CASES, LINEAR_CASES as SPLIT_LINEAR_CASES, Q8_CASES, W2_CONV_CASES, W2_LINEAR_CASES
from test_gpu_f32 import CONV_CASES as F32_CONV_CASES, MODES as F32_MODES

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
_DTN = {F16: "fp16", BF16: "bf16", F32: "fp32"}
FAMILIES = {}


class Case:
    def __init__(self, family, name, wrappers, build, dtype):
        self.family, self.name, self.wrappers, self.build, self.dtype = family, name, tuple(wrappers), build, dtype

    @property
    def id(self):
        return self.name + ("" if self.dtype is None else "-" + _DTN[self.dtype])


def case(family, name, wrappers, dtypes=(None,), **kw):
    """Register ``build(dev, dtype, **kw) -> dict(fn, operands[, expect, prefix, finite])`` as one case per dtype."""
    def deco(build):
        for dt in dtypes:
            FAMILIES.setdefault(family, []).append(Case(family, name, wrappers, lambda dev, d, b=build, k=kw: b(dev, d, **k), dt))
        return build
    return deco


def declared_wrappers():
    return {w for cases in FAMILIES.values() for c in cases for w in c.wrappers}


def _run(cuda, c):
    spec = c.build(cuda, c.dtype)
    got, rec = G.run_guarded(spec["fn"], spec["operands"], expect=spec.get("expect"), finite=spec.get("finite"))
    print(f"{c.family}/{c.id}: launched {rec.names}")
    if spec.get("workspace"):      # the case is about a workspace: the wrapper did allocate one, between guards like everything else
        assert any(r.kind == "alloc" and r.view.dtype == torch.uint8 and r.view.numel() > 0 for r in rec.arena.regions), "no workspace was allocated"
    if spec.get("prefix"):
        assert any(n.startswith(spec["prefix"]) for n in rec.names), f"no {spec['prefix']}* kernel ran: {rec.names}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _under(*ctx):
    """``fn -> fn`` run inside fresh instances of the given context managers (zero-argument factories)."""
    def wrap(f):
        def run(**kw):
            with contextlib.ExitStack() as st:
                for c in ctx:
                    st.enter_context(c())
                return f(**kw)
        return run
    return wrap


def _policy(name):
    from rsvld_amd import ops
    return {"all_split": lambda: ops.f32_split(ops.ALL_SPLIT), "unet": lambda: ops.f32_split(ops.UNET_POLICY),
            "pairs": lambda: ops.f32_split(ops.SplitPolicy(f16_weights=())), "attn16": lambda: ops.f32_split(ops.SplitPolicy(f16_inputs=("attn",))),
            "f32_onthefly": lambda: ops.f32_split(ops.SplitPolicy(impl="f32", f16_inputs=())), "fp32": lambda: ops.f32_split(None)}[name]


def _tune(**kw):
    from rsvld_amd import ops
    return lambda: ops.tuning(**kw)


# ============================================================================= convolutions
def _conv_spec(dev, xdt, B, C1, Cout, H, W, k, stride, pad, up, *, C2=0, wdt=None, rowvec=False, rv_slice=False, residual=False, norm=False,
               stats=False, out_f32=False, res_dt=None, geglu=False, alpha=1.0, beta=1.0, ctx=(), forms=(), conv_kw=None, seed=0, expect=None,
               prefix=None):
    from rsvld_amd import ops, _lib as L
    g = _gen(seed + B + C1 + C2 + Cout + H + W)
    wdt = xdt if wdt is None else wdt
    Ct = C1 + C2
    x = (torch.randn(B, H, W, C1, generator=g) * 1.5 + 0.3).to(dev, xdt)
    x2 = torch.randn(B, H, W, C2, generator=g).to(dev, xdt) if C2 else None
    w = torch.randn(Cout, Ct, k, k, generator=g) / math.sqrt(Ct * k * k)
    pc = ops.pack_conv(w, torch.randn(Cout, generator=g) * 0.1, wdt, dev, cin_split=(C1, C2) if C2 else None, geglu=geglu)
    pt, pl, pb, pr = (pad,) * 4 if isinstance(pad, int) else pad
    Hin, Win = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hin + pt + pb - k) // stride + 1, (Win + pl + pr - k) // stride + 1
    c_out = pc.cout_p // 2 if geglu else pc.cout_p
    operands = dict(x=x, x2=x2, pc=G.Op(pc, forms=forms), rowvec=None, residual=None, norm=None)
    if rowvec:
        rv = torch.randn(B, 2 * pc.cout_p if rv_slice else pc.cout_p, generator=g).to(dev)
        operands["rowvec"] = G.Op(rv[:, pc.cout_p:], view=True) if rv_slice else rv     # a slice of a wider table: poison between its rows
    if residual:
        rdt = res_dt or (F32 if out_f32 else xdt)
        operands["residual"] = torch.randn(B, Ho, Wo, c_out, generator=g).to(dev, rdt)
    if norm:
        operands["norm"] = ((1 + 0.1 * torch.randn(Ct, generator=g)).to(dev), (0.1 * torch.randn(Ct, generator=g)).to(dev), 32, 1e-5, True)
    kw = dict(stride=stride, pad=pad, upsample=up, stats=stats, out_f32=out_f32, alpha=alpha, beta=beta, act=L.ACT_GEGLU if geglu else L.ACT_NONE)
    kw.update(conv_kw or {})
    fn = _under(*ctx)(lambda x, x2, pc, rowvec, residual, norm: ops.conv2d(x, pc, x2=x2, rowvec=rowvec, residual=residual, norm=norm, **kw))
    return dict(fn=fn, operands=operands, expect=expect, prefix=prefix)


def _igemm(name, args, dtypes=(F16, BF16), **kw):
    @case("conv_igemm", name, ("conv2d",), dtypes)
    def build(dev, dt):
        B, Cin, Cout, H, W, k, stride, pad, up = args
        return _conv_spec(dev, dt, B, Cin, Cout, H, W, k, stride, pad, up, ctx=(_tune(use_halo=False),), prefix="conv_igemm", **kw)


_igemm("first_conv_cin8", CONV_CASES[1])                      # Cin 8: one 8-channel piece per tap, the rest of the K step zero-filled by predicate
_igemm("stride2_ragged_m", CONV_CASES[2])                     # M = 2 * 9 * 7 = 126 rows in a 128-row tile: rows past M re-read a valid address, never stored
_igemm("conv1x1_ragged_m", CONV_CASES[3])                     # 1x1, M = 99
_igemm("cout8", CONV_CASES[4])                                # 256x32 tile with 8 real columns: weight rows past Cout clamped, their channels never stored
_igemm("cout48", (1, 64, 48, 9, 13, 3, 1, 1, False))          # 128x64 tile, 48 real columns and M = 117
_igemm("nearest_x2", CONV_CASES[5])                           # the gather halves the coordinates: the last source row / column must not be exceeded
_igemm("two_k_groups_ragged_m", CONV_CASES[10])               # two K groups per workgroup, M = 1023: the second group's reduction through LDS
_igemm("stride2_asymmetric_pad", (1, 64, 64, 16, 16, 3, 2, (0, 0, 1, 1), False))   # the VAE's Downsample: the window leaves the image at the bottom / right only
_igemm("two_source_rowvec_slice_residual", (3, 64, 128, 12, 10, 3, 1, 1, False), C2=32, rowvec=True, rv_slice=True, residual=True,
       alpha=0.5, beta=2.0)                                   # K straddles the sources; rowvec rows 2 * Cout apart with poison between them
_igemm("out_f32_cout3", (1, 64, 3, 16, 16, 3, 1, 1, False), out_f32=True)   # pad channels 3..7 are part of the result: zero, not unwritten
_igemm("geglu_epilogue", (1, 320, 640, 1, 200, 1, 1, 0, False), geglu=True)  # value / gate pairs: 320 output columns from 640 weight rows, M = 200


def _halo(name, args, dtypes=(F16,), **kw):
    @case("conv_halo", name, ("conv2d",), dtypes)
    def build(dev, dt):
        B, C1, C2, Cout, H, W, fuse = args
        pre = "conv_halo_64" if Cout <= 64 else "conv_halo_128"
        return _conv_spec(dev, dt, B, C1, Cout, H, W, 3, 1, 1, False, C2=C2, rowvec=True, residual=True, norm=fuse,
                          ctx=(_tune(halo_min_wgs=0),), expect=pre, **kw)


_halo("ragged_h_w", HALO_CASES[1], (F16, BF16))               # 19 x 45: patch rows / columns past the image are zero-filled, pixels past it never stored
_halo("two_source_groups_straddle", HALO_CASES[2], (F16, BF16))   # GroupNorm groups straddle x | x2: the scale / shift table is indexed across the seam
_halo("w16_half_filled_tile", HALO_CASES[3])                  # W = 16 in a 32-pixel tile: half of every tile row lies past the image
_halo("cout8", HALO_CASES[4])                                 # BN = 64 with 8 real rows: "rows past Cout re-read the last row: their accumulators are never stored"
_halo("sixteen_bodies", HALO_CASES[7])                        # every steady-state prefetch slot; the last prefetch must not run past the second source
_halo("single_body", HALO_CASES[8], (F16, BF16))              # no prefetch beyond the prologue
_halo("eight_wave_ragged", HALO_CASES[10])                    # 16 x 32 pixel tiles, H = 88 = 5.5 tiles: the second sub-tile of the last row is absent
_halo("eight_wave_no_norm", HALO_CASES[11])                   # 90 x 97 without the fused norm
_halo("cout48_clamped_weight_rows", HALO_CASES[13], (F16, BF16))   # BN = 64, 48 real rows, three tile columns
_halo("stats_part_out", HALO_CASES[1], (F16, BF16), stats=True, seed=1)   # part_out [B, tiles, Cout, 2] is returned: every ragged tile must write its partials
_halo("eight_wave_stats_part_out", HALO_CASES[10], stats=True, seed=1)    # two 8 x 32 partial tiles per workgroup, the second absent on the last row


@case("conv_halo", "norm_from_producer_partials", ("conv2d",), (F16, BF16))
def _halo_partials(dev, dt):
    """The consumer's GroupNorm statistics come from the producers' epilogue partials (two producers, groups straddle): the
    partial tensors are operands of rsvld_groupnorm_scale_shift_from_partials and get guards of their own."""
    from rsvld_amd import ops
    g = _gen(21)
    B, H, W = 2, 19, 40
    with ops.tuning(halo_min_wgs=0):
        ya = ops.conv2d(torch.randn(B, H, W, 64, generator=g).to(dev, dt), ops.pack_conv(torch.randn(128, 64, 3, 3, generator=g) / 24, None, dt, dev), pad=1, stats=True)
        yb = ops.conv2d(torch.randn(B, H, W, 128, generator=g).to(dev, dt), ops.pack_conv(torch.randn(64, 128, 3, 3, generator=g) / 34, None, dt, dev), pad=1, stats=True)
    assert hasattr(ya, "_gn_part") and hasattr(yb, "_gn_part")
    pcc = ops.pack_conv(torch.randn(128, 192, 3, 3, generator=g) / 41, None, dt, dev)
    norm = ((1 + 0.1 * torch.randn(192, generator=g)).to(dev), (0.1 * torch.randn(192, generator=g)).to(dev), 32, 1e-5, True)
    fn = _under(_tune(halo_min_wgs=0))(lambda x, x2, pc, norm: ops.conv2d(x, pc, x2=x2, pad=1, norm=norm))
    return dict(fn=fn, operands=dict(x=ya, x2=yb, pc=pcc, norm=norm), expect=("groupnorm_ab_from_partials", "conv_halo_128"))


@case("conv_halo", "fused_upsample", ("conv2d",), (F16, BF16))
def _halo_up(dev, dt):    # nearest x2 folded into the patch staging: source rows (y >> 1) past H must be clamped / zero-filled
    return _conv_spec(dev, dt, 2, 128, 128, 9, 21, 3, 1, 1, True, ctx=(_tune(halo_min_wgs=0),), expect="conv_halo_128")


def _halo_w2(name, args, **kw):
    @case("conv_halo", "w2_" + name, ("conv2d",))
    def build(dev, dt):
        B, Cin, Cin2, Cout, H, W, up, use_res, use_rv, use_norm, f32_out = args
        return _conv_spec(dev, F16, B, Cin, Cout, H, W, 3, 1, 1, up, C2=Cin2, wdt=F32, rowvec=use_rv, residual=use_res, norm=use_norm, stats=True,
                          out_f32=f32_out, forms=("w2",), ctx=(_tune(halo_min_wgs=0),), expect=("conv_halo_64" if Cout <= 64 else "conv_halo_128") + "_w2", **kw)


_halo_w2("halo64_ragged_tiles", W2_CONV_CASES[0])             # 250 x 260: ragged tile rows and columns, fused norm, fp16 residual, partials out
_halo_w2("two_source_eight_wave", W2_CONV_CASES[2])           # NW = 8, norm over the concat
_halo_w2("f32_out_residual", W2_CONV_CASES[4])                # fp32 epilogue + fp32 residual, W = 250
_halo_w2("small_ragged", (2, 64, 64, 128, 19, 45, False, True, True, True, False))   # the 16-bit table's ragged row with the pair weights (twice the K per tap)


def _halo_split(name, args):
    @case("conv_halo", "split_" + name, ("conv2d",))
    def build(dev, dt):
        B, Cin, Cin2, Cout, H, W, k, stride, pad, up, use_res, use_rv, stats = args
        return _conv_spec(dev, F32, B, Cin, Cout, H, W, k, stride, pad, up, C2=Cin2, wdt=F32, rowvec=use_rv, residual=use_res, stats=stats,
                          res_dt=F32, forms=("w3",), ctx=(_policy("all_split"), _tune(split_halo_min_wgs=0)),
                          expect=("conv_halo_64" if Cout <= 64 else "conv_halo_128") + "_split")


_halo_split("halo64_ragged_tiles", SPLIT_CONV_CASES[0])       # bf16 planes lo | hi per pixel: the patch row is twice as wide, same clamps
_halo_split("two_source_eight_wave", SPLIT_CONV_CASES[2])
_halo_split("nearest_x2", SPLIT_CONV_CASES[3])
_halo_split("small_ragged", (2, 128, 64, 256, 9, 33, 3, 1, 1, False, True, True, True))


def _halo_q8(name, args):
    @case("conv_halo", "q8_" + name, ("conv2d",))
    def build(dev, dt):
        B, H, W, C1, C2, Co, use_rv, use_res = args
        return _conv_spec(dev, F32, B, C1, Co, H, W, 3, 1, 1, False, C2=C2, wdt=F32, rowvec=use_rv, residual=use_res, norm=True, stats=True,
                          res_dt=F32, alpha=0.5 if use_res else 1.0, forms=("wq8",), ctx=(_policy("unet"), _tune(split_halo_min_wgs=0)),
                          conv_kw=dict(norm_group="conv1", out_f32=False), expect=("groupnorm_apply_q8", "conv_halo_128_q8"))


_halo_q8("two_source_ragged", Q8_CASES[1])                    # 19 x 37: Q8Rows of the normalised concat, ragged tile rows and columns
_halo_q8("cout_two_and_a_half_tiles", Q8_CASES[3])            # Cout 320: the last column tile holds 64 real weight rows
_halo_q8("every_epilogue_input", Q8_CASES[0])


# ============================================================================= gemm256
def _linear_spec(dev, dt, M, K, N, act, use_res, *, mode="16", alpha=1.0, beta=1.0, bias=True, out_planes=False, seed=0):
    from rsvld_amd import ops, _lib as L
    g = torch.Generator(device=dev).manual_seed(seed + M + K + N)
    xdt = {"16": dt, "one_tile": dt, "w1": F16, "w2": F16, "split": F32}[mode]
    x = torch.randn(M, K, generator=g, device=dev).to(xdt)
    w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K))
    b = torch.randn(N, generator=g, device=dev) * 0.1 if bias else None
    pc = ops.pack_conv(w, b, dt if mode in ("16", "one_tile") else F32, dev, geglu=(act == 2))
    n_out = N // 2 if act == 2 else N
    rdt = dt if mode in ("16", "one_tile") else F32
    res = torch.randn(M, n_out, generator=g, device=dev).to(rdt) if use_res else None
    ctx, forms, sfx, kw = (), (), "", {}
    if mode == "one_tile":
        ctx = (_tune(tune=L.TUNE_GEMM_ONE_TILE),)
    elif mode == "w1":     # fp16 x fp16-rounded weights, fp32 out + fp32 residual (RSVLD_F16W1)
        ctx, forms, sfx, kw = (_policy("unet"),), ("w1",), "_w1", dict(group="ff_out")
    elif mode == "w2":     # fp16 x weight pairs [W_lo | W_hi] (RSVLD_F16W2)
        ctx, forms, sfx, kw = (_policy("pairs"),), ("w2",), "_w2", dict(out_planes=out_planes, out_group="ff")
    elif mode == "split":  # bf16 planes x weight triples (RSVLD_SPLIT)
        ctx, forms, sfx, kw = (_policy("all_split"),), ("w3",), "_split", dict(out_planes=out_planes)
        x = ops.to_planes(x)
    a = {0: L.ACT_NONE, 1: L.ACT_SILU, 2: L.ACT_GEGLU}[act]
    fn = _under(*ctx)(lambda x, pc, residual: ops.linear(x, pc, residual=residual, act=a, alpha=alpha, beta=beta, **kw))
    # (the library's plan of the layer, rsvld_plan_conv: smaller problems run the implicit-GEMM kernel of the same dtype)
    big = plan_conv(linear_desc(M, K, pc.cout_p, 0)).gemm256 != 0
    return dict(fn=fn, operands=dict(x=x, pc=G.Op(pc, forms=forms), residual=res), expect="gemm_256x256" + sfx if big else None,
                prefix=None if big else "conv_igemm")


def _gemm(name, args, dtypes=(F16,), **kw):
    @case("gemm256", name, ("linear",), dtypes)
    def build(dev, dt):
        M, K, N, act, use_res = args
        return _linear_spec(dev, dt, M, K, N, act, use_res, **kw)


_gemm("ragged_m_tile", GEMM_CASES[0], (F16, BF16))            # M = 4160: 64 real rows in the last tile; "rows past the end re-read a valid address (never stored)"
_gemm("ragged_n_8_columns_one_k_tile", GEMM_CASES[1], (F16, BF16))   # N = 3848: a tile of 8 columns; "channels past N are never stored"; residual rows read under the same mask
_gemm("geglu", GEMM_CASES[3])                                 # value / gate pairs: the output is half as wide as the weight
_gemm("persistent_ragged_n", GEMM_CASES[4], (F16, BF16))      # 289 tiles on 256 workgroups, N = 4104
_gemm("persistent_n_mod_256_is_128", GEMM_CASES[6])           # N = 640: the last column tile is half real
_gemm("persistent_geglu_ragged_m", GEMM_CASES[7])             # M = 16640
_gemm("half_tiles", GEMM_CASES[9])                            # every workgroup ends on a 128-row half tile
_gemm("half_tiles_lower_half_beyond_m", GEMM_CASES[10], (F16, BF16))   # the last tile row has 128 rows: its lower halves lie beyond M and must not be touched
_gemm("one_tile_form_alpha_beta_residual", (8448, 384, 2304, 0, True), mode="one_tile", alpha=0.5, beta=2.0)
_gemm("persistent_alpha_beta_residual", (8448, 384, 2304, 0, True), alpha=0.5, beta=2.0)
_gemm("one_tile_form_no_bias", (8192, 640, 2048, 0, False), mode="one_tile", bias=False)
# (8 269 x 2 560 -> 640 is 99 tiles, below the gemm256 threshold: the implicit-GEMM kernel runs and the label says so; either way the ragged last row tile)
_gemm("w1_fp32_residual_8269_rows", (W2_LINEAR_CASES[1][0], W2_LINEAR_CASES[1][1], W2_LINEAR_CASES[1][2], 0, True), mode="w1", alpha=0.5)
_gemm("w1_ragged_rows_and_column_tile", (20000, 640, 640, 0, True), mode="w1", alpha=0.5)
_gemm("w2_pairs_8269_rows", (W2_LINEAR_CASES[1][0], W2_LINEAR_CASES[1][1], W2_LINEAR_CASES[1][2], 0, True), mode="w2", alpha=0.5)
_gemm("w2_pairs_ragged_rows_and_column_tile", (W2_LINEAR_CASES[3][0], W2_LINEAR_CASES[3][1], W2_LINEAR_CASES[3][2], 0, True), mode="w2", alpha=0.5)
_gemm("w2_pairs_geglu_f16_out", (W2_LINEAR_CASES[0][0], W2_LINEAR_CASES[0][1], W2_LINEAR_CASES[0][2], 2, False), mode="w2", out_planes=True)
_gemm("split_triples_ragged_rows_residual", (SPLIT_LINEAR_CASES[1][0], SPLIT_LINEAR_CASES[1][1], SPLIT_LINEAR_CASES[1][2], 0, True), mode="split", alpha=0.5)
_gemm("split_triples_n320", (SPLIT_LINEAR_CASES[3][0], SPLIT_LINEAR_CASES[3][1], SPLIT_LINEAR_CASES[3][2], 0, True), mode="split", alpha=0.5)
_gemm("split_triples_planes_out", (SPLIT_LINEAR_CASES[0][0], SPLIT_LINEAR_CASES[0][1], SPLIT_LINEAR_CASES[0][2], 0, False), mode="split", out_planes=True)


# ============================================================================= attention
@contextlib.contextmanager
def _d64(kind):
    from rsvld_amd import devtools
    devtools.d64_kernel(kind)
    try:
        yield
    finally:
        devtools.d64_kernel("")


@contextlib.contextmanager
def _d512(kind):
    from rsvld_amd import devtools
    devtools.d512_kernel(kind)
    try:
        yield
    finally:
        devtools.d512_kernel("")


def _attn_operands(dev, dt, B, heads, Nq, Nk, D, *, shared=False, fused=True, planes=False, amp=1.0, seed=0):
    """q | k | v: column slices of ONE fused projection (q | k | v when Nq == Nk, else q alone and k | v fused), placed with poison in
    the gaps between their rows -- the neighbours of a token's q are NaN, not its k; ``shared``: keys and values are one tensor."""
    from rsvld_amd import ops
    g = _gen(seed + Nq * 7 + Nk + heads)
    HD = heads * D
    mk = lambda *s: (torch.randn(*s, generator=g) * amp).to(dev, F32 if planes else dt)
    wrap = (lambda t: ops.to_planes(t)) if planes else (lambda t: t)
    if shared:
        q, x = wrap(mk(B, Nq, HD)), wrap(mk(B, Nk, HD))
        return dict(q=q, k=x, v=x)
    if not fused:
        return dict(q=wrap(mk(B, Nq, HD)), k=wrap(mk(B, Nk, HD)), v=wrap(mk(B, Nk, HD)))
    if Nq == Nk:
        qkv = wrap(mk(B, Nq, 3 * HD))
        return dict(q=G.Op(qkv[..., :HD], view=True), k=G.Op(qkv[..., HD:2 * HD], view=True), v=G.Op(qkv[..., 2 * HD:], view=True))
    kv = wrap(mk(B, Nk, 2 * HD))
    return dict(q=wrap(mk(B, Nq, HD)), k=G.Op(kv[..., :HD], view=True), v=G.Op(kv[..., HD:], view=True))


def _attn_fn(heads, *ctx, scale=None):
    from rsvld_amd import ops
    return _under(*ctx)(lambda q, k, v: ops.attention(q, k, v, heads, scale))


ATTN64, ATTN512 = [], []     # (form, shape) / (name, shape, kernel, plan_div, shared): walked on the CPU by tests/test_attn_plan_cases.py


def _attn64(form, shape, dtypes=(F16,)):
    B, heads, Nq, Nk = shape
    ATTN64.append((form, shape))
    @case("attention", f"d64{form}_B{B}h{heads}_{Nq}x{Nk}", ("attention",), dtypes)
    def build(dev, dt):
        return dict(fn=_attn_fn(heads, lambda: _d64(form)), operands=_attn_operands(dev, dt, B, heads, Nq, Nk, 64), prefix="attention_d64")


for _form in ("b", "c"):       # the two bit-identical d = 64 forms: each has its own K / V tile loads and its own store guard
    _attn64(_form, (1, 20, 64, 77), (F16, BF16))   # Nk = 77: 13 real keys in the second tile: "rows past Nk re-read the last key and are masked in the softmax"
    _attn64(_form, (2, 5, 100, 333))               # Nq and Nk ragged, batch 2
    _attn64(_form, (3, 2, 1, 1))                   # one query, one key
    _attn64(_form, (1, 1, 513, 129))               # one row / one key past a tile edge
    _attn64(_form, (1, 2, 256, 256))               # exact tiles, q | k | v slices of one fused tensor


def attn512_plan(name, shape, kernel, plan, shared):
    """The library's plan of an ``_attn512`` case, checked against what the case's NAME claims: ``split_kv`` = key ranges merged from a
    workspace, ``unsplit`` = one range and no workspace."""
    B, Nq, Nk = shape
    pl = attn_plan(B, 1, Nq, Nk, 512, plan_div=plan, tune={"rows": 4, "dsplit": 5, "": 0}[kernel], shared=shared)
    assert (pl.nsplit > 1) == (pl.ws_bytes > 0)
    if "split_kv" in name or "unsplit" in name:
        assert (pl.nsplit > 1) == ("split_kv" in name), (name, pl.nsplit)
    return pl


def _attn512(name, shape, dtypes=(F16,), kernel="", plan=1, shared=False, **okw):
    B, Nq, Nk = shape
    ATTN512.append((name, shape, kernel, plan, shared))
    @case("attention", f"d512_{name}_B{B}_{Nq}x{Nk}", ("attention",), dtypes)
    def build(dev, dt):
        from rsvld_amd import ops
        # a plan with key ranges is a case about its workspace as well: the partials are a guarded allocation
        return dict(fn=_attn_fn(1, lambda: _d512(kernel), lambda: ops.plan_units(plan)), operands=_attn_operands(dev, dt, B, 1, Nq, Nk, 512, shared=shared, **okw),
                    expect="attention_d512", workspace=attn512_plan(name, shape, kernel, plan, shared).ws_bytes > 0)


_attn512("two_tensor_fused_qkv", (2, 144, 144), (F16, BF16))             # q | k | v slices, token stride 1536
_attn512("two_tensor_ragged", (1, 100, 333), (F16, BF16))                # k | v fused, 13 keys in the last tile
_attn512("two_tensor_split_kv_ragged_last_range", (1, 300, 2500))        # split-KV: the partials workspace is a guarded allocation, the last key range is short
_attn512("one_query_one_key", (1, 1, 1))
_attn512("shared_tile_ragged", (1, 33, 95), (F16, BF16), shared=True)    # attn_d512b with the shared K = V tile, read row-wise and transposed
_attn512("shared_tile_split_kv_ragged_last_range", (1, 300, 2500), shared=True)
_attn512("shared_tile_rows_kernel", (1, 300, 4096 + 17), shared=True, kernel="rows")
_attn512("shared_tile_dsplit_kernel", (1, 300, 4096 + 17), (F16, BF16), shared=True, kernel="dsplit")   # attn_d512d: P exchanged through LDS
_attn512("shared_tile_dsplit_unsplit_partial_query_tile", (1, 24576 + 77, 2048 + 5), shared=True, kernel="dsplit")
_attn512("shared_tile_dsplit_plan_div", (2, 640, 8192 + 31), shared=True, kernel="dsplit", plan=2)       # planned per image


def _attn_split(name, shape, D, policy, *ctx, expect=None, prefix=None, **okw):
    B, heads, Nq, Nk = shape
    @case("attention", f"{name}_B{B}h{heads}_{Nq}x{Nk}", ("attention",))
    def build(dev, dt):
        return dict(fn=_attn_fn(heads, _policy(policy), *ctx, scale=D ** -0.5), operands=_attn_operands(dev, F16, B, heads, Nq, Nk, D, planes=True, **okw),
                    expect=expect, prefix=prefix)


_attn_split("split_d64_fused_cross", (2, 20, 200, 77), 64, "all_split", expect="attention_split_d64_cross")   # k | v planes slices of one fused tensor
_attn_split("split_d64_fused_ragged_peaky", (1, 3, 129, 65), 64, "all_split", expect="attention_split_d64_cross", amp=3.0)
_attn_split("split_d64_fused_qkv", (2, 5, 300, 300), 64, "all_split", expect="attention_split_d64")
_attn_split("split_d512_fused_shared", (2, 1, 200, 333), 512, "all_split", _tune(split_d512_fused_min=1), expect="attention_split_d512", shared=True, amp=0.7)
_attn_split("split_d512_fused_one_tile", (1, 1, 64, 64), 512, "all_split", _tune(split_d512_fused_min=1), expect="attention_split_d512", shared=True, amp=0.7)
# the GEMM form: keys padded to 8 in the triples, S and P blocks per 256 query rows -- every workspace is a guarded allocation
_attn_split("split_gemm_form", (1, 1, 33, 1000), 512, "all_split", expect=("attention_split_gemm_qk_d512", "attention_split_softmax", "attention_split_gemm_pv_d512"),
            fused=False, amp=0.5)
_attn_split("split_gemm_form_keys_padded_to_8", (1, 1, 40, 77), 512, "all_split", expect="attention_split_softmax", fused=False, amp=0.5)   # 3 pad keys: zero rows, masked columns
_attn_split("split_gemm_form_shared_d128", (2, 1, 64, 64), 128, "all_split", expect="attention_split_gemm_pv_d128", shared=True, amp=0.5)
# the fp16 hand-over composition: planes -> fp16 (channel slices read in place) -> the 16-bit kernels -> planes / fp16
_attn_split("handover_f16_d64_to_planes", (1, 20, 300, 77), 64, "attn16", expect=("planes_to_f16", "attention_d64_cross", "f16_to_planes"))
_attn_split("handover_f16_d64_fused_qkv", (2, 5, 1024, 1024), 64, "unet", expect=("planes_to_f16", "attention_d64"))
_attn_split("handover_f16_d512_shared", (1, 1, 1000, 1000), 512, "unet", expect=("planes_to_f16", "attention_d512"), shared=True)


def _attn_f32(mode, shape, D):
    B, heads, Nq, Nk = shape
    @case("f32_family", f"attention_{mode}_B{B}h{heads}_{Nq}x{Nk}_d{D}", ("attention",))
    def build(dev, dt):
        pol = {"fp32": "fp32", "split": "all_split", "f32_onthefly": "f32_onthefly"}[mode]
        pre = {"fp32": "attention_f32_d", "split": "attention_split", "f32_onthefly": "attention_f32_split_d"}[mode]
        return dict(fn=_attn_fn(heads, _policy(pol)), operands=_attn_operands(dev, F32, B, heads, Nq, Nk, D), prefix=pre)


for _mode in list(F32_MODES) + ["f32_onthefly"]:      # test_gpu_f32.MODES + round 3's on-the-fly split inside the fp32 kernels
    _attn_f32(_mode, (1, 2, 45, 77), 64)              # "clamped rows carry P = 0": 45 queries, 77 keys
    _attn_f32(_mode, (1, 1, 33, 1000), 512)
    _attn_f32(_mode, (2, 1, 64, 64), 128)             # q | k | v slices of one fused fp32 tensor


# ============================================================================= fp32 family: convolutions and norms
def _conv_f32(mode, name, args):
    @case("f32_family", f"conv_{mode}_{name}", ("conv2d",))
    def build(dev, dt):
        B, Cin, Cout, H, W, k, stride, pad, up, use_res, silu = args
        from rsvld_amd import _lib as L
        return _conv_spec(dev, F32, B, Cin, Cout, H, W, k, stride, pad, up, wdt=F32, residual=use_res, res_dt=F32,
                          ctx=(_policy({"fp32": "fp32", "f32_onthefly": "f32_onthefly"}[mode]),), conv_kw=dict(act=L.ACT_SILU if silu else L.ACT_NONE, out_f32=False, stats=False),
                          expect="conv_f32" if mode == "fp32" else "conv_f32_split")


for _mode in ("fp32", "f32_onthefly"):
    _conv_f32(_mode, "stride2_asymmetric_ragged", F32_CONV_CASES[2])
    _conv_f32(_mode, "cout8", F32_CONV_CASES[4])
    _conv_f32(_mode, "nearest_x2", F32_CONV_CASES[5])
    _conv_f32(_mode, "multiples_of_8_residual_silu", F32_CONV_CASES[6])


@case("f32_family", "conv_fp32_two_source_rowvec", ("conv2d",))
def _conv_f32_two(dev, dt):
    return _conv_spec(dev, F32, 2, 64, 96, 9, 7, 3, 1, 1, False, C2=40, wdt=F32, rowvec=True, rv_slice=True, ctx=(_policy("fp32"),), expect="conv_f32")


@case("f32_family", "linear_fp32_geglu", ("linear",))
def _lin_f32_geglu(dev, dt):
    from rsvld_amd import ops, _lib as L
    g = _gen(11)
    pc = ops.pack_conv(torch.randn(256, 64, generator=g) / 8, torch.randn(256, generator=g) * 0.1, F32, dev, geglu=True)
    return dict(fn=lambda x, pc: ops.linear(x, pc, act=L.ACT_GEGLU), operands=dict(x=torch.randn(300, 64, generator=g).to(dev), pc=pc), expect="conv_f32")


@case("f32_family", "split_igemm_small_m", ("linear",))
def _lin_split_small(dev, dt):       # rows = 300: the implicit-GEMM kernel's RSVLD_SPLIT instantiation
    spec = _linear_spec(dev, F16, 300, 640, 640, 0, True, mode="split", alpha=0.5)
    spec["expect"] = "conv_igemm_split"
    return spec


@case("f32_family", "split_igemm_stride2_ragged", ("conv2d",))
def _conv_split_igemm(dev, dt):
    B, Cin, Cin2, Cout, H, W, k, stride, pad, up, use_res, use_rv, stats = SPLIT_CONV_CASES[5]
    return _conv_spec(dev, F32, B, Cin, Cout, H, W, k, stride, pad, up, wdt=F32, forms=("w3",), ctx=(_policy("all_split"),), expect="conv_igemm_split")


@case("f32_family", "w2_igemm_small_m", ("linear",))
def _lin_w2_small(dev, dt):
    spec = _linear_spec(dev, F16, 300, 640, 640, 0, True, mode="w2", alpha=0.5)
    spec["expect"] = None
    spec["prefix"] = "conv_igemm"
    return spec


# ============================================================================= norms
def _gn_inputs(dev, dt, B, C1, C2, H, W, seed=0):
    g = _gen(seed + C1 + C2)
    x = (torch.randn(B, H, W, C1, generator=g) * 2 + 0.5).to(dev, dt)
    x2 = torch.randn(B, H, W, C2, generator=g).to(dev, dt) if C2 else None
    gamma, beta = (1 + 0.1 * torch.randn(C1 + C2, generator=g)).to(dev), (0.1 * torch.randn(C1 + C2, generator=g)).to(dev)
    return g, x, x2, gamma, beta


def _gn(name, args, dtypes=(F16,), family="norms", policy=None, expect=None, **gkw):
    @case(family, "group_norm_" + name, ("group_norm",), dtypes)
    def build(dev, dt):
        from rsvld_amd import ops
        B, C1, C2, H, W, G_, silu = args
        _, x, x2, gamma, beta = _gn_inputs(dev, dt or F32, B, C1, C2, H, W)
        ctx = () if policy is None else (_policy(policy),)
        fn = _under(*ctx)(lambda x, x2, gamma, beta: ops.group_norm(x, gamma, beta, G_, 1e-5, x2=x2, silu=silu, **gkw))
        return dict(fn=fn, operands=dict(x=x, x2=x2, gamma=gamma, beta=beta), expect=expect)


_gn("63_pixels_10_channels_per_group", GN_CASES[1], (F16, BF16), expect="groupnorm(3 kernels)")   # 9 x 7 pixels: the pixel loop's tail
_gn("16_pixels_wide_groups", GN_CASES[3], expect="groupnorm(3 kernels)")
_gn("one_launch_form", GN_CASES[6], (F16, BF16), expect="groupnorm(3 kernels)")                   # one workgroup per image x group, slab in registers
_gn("one_launch_two_source_ragged", GN_CASES[7], (F16, BF16), expect="groupnorm(3 kernels)")      # 17 x 19 pixels, groups on either side of the seam
_gn("chunked_form", GN_CASES[8], expect="groupnorm(3 kernels)")                                   # 4 x 512 x 64 x 64: statistics over chunks + workspace
_gn("chunked_form_40x40", GN_CASES[4], (F16, BF16), expect="groupnorm(3 kernels)")
_gn("fp32", (2, 128, 0, 19, 23, 32, True), (None,), family="f32_family", expect=("groupnorm_stats_f32", "groupnorm_apply_f32"))
_gn("fp32_ragged_pixels", (1, 32, 0, 70, 66, 32, True), (None,), family="f32_family", expect="groupnorm_apply_f32")
_gn("split_fp32_out", (2, 128, 0, 19, 23, 32, True), (None,), policy="all_split", expect=("groupnorm_stats_split", "groupnorm_apply_split"))
_gn("split_planes_out_two_source", (1, 32, 32, 70, 66, 32, True), (None,), policy="all_split", expect="groupnorm_apply_split", planes=True)
_gn("split_f16_out", (2, 640, 0, 40, 24, 32, True), (None,), policy="unet", expect="groupnorm_apply_split", planes=True, group="ff")


def _gn_mod(name, dtypes, family="norms", policy=None, C1=320, C2=0, expect=None):
    @case(family, "group_norm_zerosft_" + name, ("group_norm",), dtypes)
    def build(dev, dt):
        """ZeroSFT: scale | shift are the two channel halves of ONE stacked tensor; each is placed with poison where the other lay."""
        from rsvld_amd import ops
        B, H, W = 2, 6, 5
        g, x, x2, gamma, beta = _gn_inputs(dev, dt or F32, B, C1, C2, H, W, seed=3)
        Cc = C1 + C2
        gb = (torch.randn(B, H, W, 2 * Cc, generator=g) * 0.3).to(dev, dt or F32)
        ctx = () if policy is None else (_policy(policy),)
        fn = _under(*ctx)(lambda x, x2, gamma, beta, sc, sh: ops.group_norm(x, gamma, beta, 32, 1e-5, x2=x2, mod_scale1p=sc, mod_shift=sh))
        return dict(fn=fn, operands=dict(x=x, x2=x2, gamma=gamma, beta=beta, sc=G.Op(gb[..., :Cc], view=True), sh=G.Op(gb[..., Cc:], view=True)), expect=expect)


_gn_mod("stacked", (F16, BF16), expect="groupnorm(3 kernels)")
_gn_mod("fp32_two_source", (None,), family="f32_family", C1=64, C2=32, expect="groupnorm_apply_f32")     # concat_c_f32, then statistics, then apply
_gn_mod("split", (None,), policy="all_split", expect="groupnorm_apply_split")


def _gn_stats(name, args, dtypes, family="norms", policy=None):
    @case(family, "group_norm_stats_" + name, ("group_norm_stats",), dtypes)
    def build(dev, dt):
        from rsvld_amd import ops
        B, C1, C2, H, W, G_, _ = args
        _, x, x2, _, _ = _gn_inputs(dev, dt or F32, B, C1, C2, H, W, seed=5)
        ctx = () if policy is None else (_policy(policy),)
        return dict(fn=_under(*ctx)(lambda x, x2: ops.group_norm_stats(x, G_, x2=x2)), operands=dict(x=x, x2=x2))


_gn_stats("two_source_ragged", GN_CASES[7], (F16, BF16))
_gn_stats("chunked", GN_CASES[8], (F16,))
_gn_stats("fp32", (1, 256, 0, 130, 70, 32, True), (None,), family="f32_family")
_gn_stats("split_two_source", (1, 32, 32, 70, 66, 32, True), (None,), policy="all_split")


def _gn_apply(name, args, dtypes, family="norms", policy=None, mod=False, **akw):
    @case(family, "group_norm_apply_" + name, ("group_norm_apply",), dtypes)
    def build(dev, dt):
        from rsvld_amd import ops
        B, C1, C2, H, W, G_, silu = args
        g, x, x2, gamma, beta = _gn_inputs(dev, dt or F32, B, C1, C2, H, W, seed=6)
        st = torch.stack([torch.randn(B, G_, generator=g), torch.rand(B, G_, generator=g) + 0.5], -1).to(dev)      # supplied statistics (the tiled VAE)
        ctx = () if policy is None else (_policy(policy),)
        operands = dict(x=x, x2=x2, st=st, gamma=gamma, beta=beta, sc=None, sh=None)
        if mod:
            gb = (torch.randn(B, H, W, 2 * (C1 + C2), generator=g) * 0.3).to(dev)
            operands.update(sc=G.Op(gb[..., :C1 + C2], view=True), sh=G.Op(gb[..., C1 + C2:], view=True))
        fn = _under(*ctx)(lambda x, x2, st, gamma, beta, sc, sh: ops.group_norm_apply(x, st, gamma, beta, G_, 1e-5, x2=x2, silu=silu, mod_scale1p=sc, mod_shift=sh, **akw))
        return dict(fn=fn, operands=operands)


_gn_apply("two_source_ragged", GN_CASES[7], (F16, BF16))
_gn_apply("fp32_modulated", (2, 128, 0, 19, 23, 32, False), (None,), family="f32_family", mod=True)
_gn_apply("split_planes", (2, 128, 0, 19, 23, 32, True), (None,), policy="all_split", planes=True)


def _ln(name, rows, Cc, dtypes, family="norms", policy=None, expect=None, **lkw):
    @case(family, f"layer_norm_{name}_{rows}x{Cc}", ("layer_norm",), dtypes)
    def build(dev, dt):
        from rsvld_amd import ops
        g = torch.Generator(device=dev).manual_seed(Cc)
        x = (torch.randn(rows, Cc, generator=g, device=dev) * 1.5 + 0.3).to(dt or F32)
        gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g, device=dev), 0.1 * torch.randn(Cc, generator=g, device=dev)
        ctx = () if policy is None else (_policy(policy),)
        return dict(fn=_under(*ctx)(lambda x, gamma, beta: ops.layer_norm(x, gamma, beta, 1e-5, **lkw)), operands=dict(x=x, gamma=gamma, beta=beta), expect=expect)


# launch_layernorm's bands (C <= 1024 / 1536 / 2048 / 4096) cap their grids at 65 536 / 49 152 / 32 768 / 16 384 rows: ONE row past the
# cap is the grid-stride loop's second pass with a single live row
_ln("one_past_the_cap", 65536 + 1, 1024, (F16, BF16))
_ln("one_past_the_cap", 49152 + 1, 1288, (F16,))
_ln("one_past_the_cap", 32768 + 1, 2048, (BF16,))
_ln("one_past_the_cap", 16384 + 1, 4096, (F16, BF16))
_ln("ragged_channels", 111, 320, (F16, BF16))
_ln("fp32", 150, 640, (None,), family="f32_family", expect="layernorm_f32")
_ln("split_fp32_out", 6144 + 357, 1288, (None,), policy="all_split", expect="layernorm_split")
_ln("split_planes_out", 6144 + 1, 1024, (None,), policy="all_split", expect="layernorm_split", planes=True)
_ln("split_planes_out", 3072 + 1, 4096, (None,), policy="all_split", expect="layernorm_split", planes=True)
_ln("split_f16_out", 6144 + 357, 2048, (None,), policy="unet", expect="layernorm_split", planes=True, group="qkv")


# ============================================================================= decode path
def _gemv(N, K, dtypes=(F16, BF16)):
    @case("decode", f"gemv_{N}x{K}", ("gemv",), dtypes)
    def build(dev, dt):        # "rows past N re-read the last row, never stored"; K = 520 / 8: the K tail of the 16-byte loads
        from rsvld_amd import ops
        g = _gen(N + K)
        w, x, b = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, dt), torch.randn(K, generator=g).to(dev, dt), (torch.randn(N, generator=g) * 0.1).to(dev, dt)
        return dict(fn=lambda w, x, b: ops.gemv(w, x, b), operands=dict(w=w, x=x, b=b), expect="gemv")

    @case("decode", f"gemv_fused_{N}x{K}", ("gemv_fused",), dtypes)
    def build2(dev, dt):
        from rsvld_amd import ops
        g = _gen(N + K + 1)
        w, x = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, dt), (torch.randn(K, generator=g) * 2).to(dev, dt)
        nw, res, gu = (torch.randn(K, generator=g) * 0.2 + 1).to(dev, dt), torch.randn(N, generator=g).to(dev, dt), torch.randn(2 * K, generator=g).to(dev, dt)
        def fn(w, x, nw, res, gu):       # the RMSNorm prologue, the residual epilogue and the SwiGLU prologue (x = [gate | up], 2 K elements)
            return (ops.gemv_fused(w, x, None, norm=(nw, 1e-5)), ops.gemv_fused(w, x, None, residual=res), ops.gemv_fused(w, gu, None, glu=True, residual=res))
        return dict(fn=fn, operands=dict(w=w, x=x, nw=nw, res=res, gu=gu), expect="gemv")


_gemv(1003, 520)
_gemv(17, 8)
_gemv(4096, 4096, (F16,))


def _decode(name, pos, dtypes=(F16,), poison_tail=False):
    @case("decode", f"llama_decode_attention_{name}", ("llama_decode_attention",), dtypes)
    def build(dev, dt):
        """The caches are updated at ``pos`` and only there (the in-place mask); the scratch ``ws`` is allocated under the proxy: poison,
        "no initial state".  ``poison_tail``: every slot beyond ``pos`` holds 0xFF bytes, as a static cache that is ``torch.empty``
        beyond its prefix may -- "rows past the prefix re-read its last row"."""
        from rsvld_amd import ops
        nq, nkv, hd, max_len = 8, 2, 128, 777
        g = _gen(pos + 1)
        qkv = torch.randn((nq + 2 * nkv) * hd, generator=g).to(dev, dt)
        kc, vc = torch.randn(nkv, max_len, hd, generator=g).to(dev, dt), torch.randn(nkv, max_len, hd, generator=g).to(dev, dt)
        if poison_tail:
            kc.view(torch.int16)[:, pos + 1:] = -1
            vc.view(torch.int16)[:, pos + 1:] = -1
        ang = torch.rand(hd // 2, generator=g) * 6
        cos, sin = torch.cat([ang.cos(), ang.cos()]).to(dev, dt), torch.cat([ang.sin(), ang.sin()]).to(dev, dt)
        mask = torch.zeros(nkv, max_len, hd, dtype=torch.bool)
        mask[:, pos] = True
        fn = lambda qkv, cos, sin, p, kc, vc: ops.llama_decode_attention(qkv, cos, sin, p, kc, vc, nq, nkv, hd ** -0.5)
        return dict(fn=fn, operands=dict(qkv=qkv, cos=cos, sin=sin, p=torch.tensor([pos], device=dev), kc=G.Op(kc, inplace=mask), vc=G.Op(vc, inplace=mask)),
                    expect="llama_decode_attention")


_decode("pos0", 0, (F16, BF16))
_decode("pos255", 255)
_decode("pos256", 256)                       # the first key of the second 256-key chunk
_decode("last_slot", 776, (F16, BF16))       # the write lands flush against the end of both caches
_decode("pos300_poisoned_tail", 300, (F16, BF16), poison_tail=True)
_decode("pos0_poisoned_tail", 0, poison_tail=True)


def _linear_small(rows, in_f, out_f, bias):
    @case("decode", f"linear_small_{rows}x{in_f}to{out_f}", ("linear_small",))
    def build(dev, dt):
        from rsvld_amd import ops
        g = _gen(rows * 1000 + in_f)
        x, w = (torch.randn(rows, in_f, generator=g) * 2).to(dev), (torch.randn(out_f, in_f, generator=g) / math.sqrt(in_f)).to(dev)
        b = torch.randn(out_f, generator=g).to(dev) if bias else None
        return dict(fn=lambda x, w, b: ops.linear_small(x, w, b, 1, 1), operands=dict(x=x, w=w, b=b))


_linear_small(3, 70, 13, True)
_linear_small(257, 323, 6, False)
_linear_small(1, 1, 1, True)
_linear_small(5, 1280, 7, True)


# ============================================================================= small kernels
def _small(name, wrappers, dtypes=(None,)):
    return case("small", name, wrappers, dtypes)


SHAPE = (2, 4, 400, 333)     # 1 065 600 elements: past the 4096 x 256 grid of the element-wise kernels (test_gpu_small_ops.SHAPE)


def _r(g, dev, shape=SHAPE, s=1.0):
    return torch.randn(shape, generator=g, device=dev) * s


@_small("nchw_to_nhwc_fresh_pad_channels", ("nchw_to_nhwc",), (F16, BF16, F32))
def _s_nchw(dev, dt):        # 5 channels into 8: the pad channels are zeroed by the kernel (zero = 1), 33 x 47 pixels
    from rsvld_amd import ops
    src = _r(torch.Generator(device=dev).manual_seed(9), dev, (2, 5, 33, 47))
    return dict(fn=lambda src: ops.nchw_to_nhwc(src, dt, scale=0.18215), operands=dict(src=src))


@_small("nchw_to_nhwc_window_c_off", ("nchw_to_nhwc",), (F16, BF16, F32))
def _s_nchw_off(dev, dt):    # into channels [6, 11) of an existing 16-channel tensor: those may change, every other byte of ``out`` may not
    from rsvld_amd import ops
    src = _r(torch.Generator(device=dev).manual_seed(9), dev, (2, 5, 33, 47))
    out = torch.full((2, 33, 47, 16), 3.0, device=dev, dtype=dt)
    mask = torch.zeros(out.shape, dtype=torch.bool)
    mask[..., 6:11] = True
    return dict(fn=lambda src, out: ops.nchw_to_nhwc(src, dt, c_off=6, out=out), operands=dict(src=src, out=G.Op(out, inplace=mask)))


@_small("nhwc_to_nchw_c_off", ("nhwc_to_nchw",), (F16, BF16, F32))
def _s_nhwc(dev, dt):
    from rsvld_amd import ops
    x = _r(torch.Generator(device=dev).manual_seed(10), dev, (2, 33, 47, 24)).to(dt)
    return dict(fn=lambda x: ops.nhwc_to_nchw(x, channels=5, c_off=8), operands=dict(x=x))


@_small("concat_c", ("concat_c",), (F16, BF16, F32))
def _s_concat(dev, dt):      # 9 000 rows x (640 + 384): past the grid; fp32: 70 rows x (64 + 40)
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    rows, ca, cb = (9000, 640, 384) if dt != F32 else (70, 64, 40)
    return dict(fn=lambda a, b: ops.concat_c(a, b), operands=dict(a=_r(g, dev, (rows, ca)).to(dt), b=_r(g, dev, (rows, cb)).to(dt)))


@_small("axpby", ("axpby",), (F16, BF16, F32))
def _s_axpby(dev, dt):       # 9 000 008 elements (16-bit: past the grid, a last vector of 8); fp32: 1003
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(8)
    n = 9000008 if dt != F32 else 1003
    return dict(fn=lambda a, b: ops.axpby(a, b, 0.7, 0.3), operands=dict(a=_r(g, dev, (n,)).to(dt), b=_r(g, dev, (n,)).to(dt)))


@_small("geglu", ("geglu",), (F16, BF16))
def _s_geglu(dev, dt):       # 6 600 x 1 280 outputs: the grid-stride loop's last pass
    from rsvld_amd import ops
    x = _r(torch.Generator(device=dev).manual_seed(7), dev, (6600, 2 * 1280)).to(dt)
    return dict(fn=lambda x: ops.geglu(x), operands=dict(x=x))


@_small("ddpm_step", ("ddpm_step",))
def _s_ddpm(dev, dt):        # fp32 NCHW x with NHWC eps of 8 channels (3 used): the channel window of eps
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(4)
    x, eps, nz = _r(g, dev, (2, 3, 10, 12)), _r(g, dev, (2, 10, 12, 8)), _r(g, dev, (2, 3, 10, 12))
    fn = lambda x, eps, nz: (ops.ddpm_step(x, eps, nz, 1.3, 0.8, 0.4, 0.6, 0.05), ops.ddpm_step(x, eps, None, 1.3, 0.8, 0.4, 0.6, 0.0))
    return dict(fn=fn, operands=dict(x=x, eps=eps, nz=nz))


@_small("sampler_elementwise_past_the_grid", ("lerp_f32", "axpy_f32", "add_f32", "euler_step", "denoiser_out"))
def _s_sampler(dev, dt):
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(11)
    a, b, c, net = _r(g, dev), _r(g, dev, s=3.0), _r(g, dev, s=0.5), _r(g, dev, (2, 400, 333, 8))
    def fn(a, b, c, net):
        return (ops.lerp_f32(a, b, 7.5), ops.axpy_f32(a, b, -0.3), ops.axpy_f32(None, b, 1.7), ops.add_f32(a, b), ops.euler_step(a, b, None, 0.3, 2.5, -0.4),
                ops.euler_step(a, b, c, 0.3, 2.5, -0.4), ops.denoiser_out(net, a, 0.7, 0.2))
    return dict(fn=fn, operands=dict(a=a, b=b, c=c, net=net))


@_small("absdiff_sums_past_the_chunk_cap", ("absdiff_sums",), (F16, BF16, F32))
def _s_absdiff(dev, dt):     # 16-bit: n8 / 256 vectors past the 256-chunk cap, a guarded workspace; fp32: 4 x 20 000
    from rsvld_amd import ops
    rows, n = (2, 4194304 + 8 * 2049 * 13) if dt != F32 else (4, 20000)
    g = torch.Generator(device=dev).manual_seed(n)
    a = _r(g, dev, (rows, n)).to(dt)
    b = (a.float() + 0.05 * _r(g, dev, (rows, n))).to(dt)
    return dict(fn=lambda a, b: ops.absdiff_sums(a, b), operands=dict(a=a, b=b))


@_small("absdiff_sums_three_vectors", ("absdiff_sums",), (F16,))
def _s_absdiff_small(dev, dt):
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(24)
    return dict(fn=lambda a, b: ops.absdiff_sums(a, b), operands=dict(a=_r(g, dev, (3, 24)).to(dt), b=_r(g, dev, (3, 24)).to(dt)))


@_small("gaussian_sample", ("gaussian_sample",), (F16, BF16, F32))
def _s_gauss(dev, dt):       # m_c = 12 > 2 C = 8: trailing channels the kernel must skip; with noise and as mode()
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(3)
    mom, noise = _r(g, dev, (2, 5, 37, 12)).to(dt), _r(g, dev, (2, 4, 5, 37))
    return dict(fn=lambda mom, noise: (ops.gaussian_sample(mom, 4, noise, 0.18215), ops.gaussian_sample(mom, 4, None, 0.18215)), operands=dict(mom=mom, noise=noise))


def _tile_blend(name, y0, x0):
    @_small(f"tile_blend_accumulate_{name}", ("tile_blend_accumulate",))
    def build(dev, dt):      # acc / cnt change inside the window and only there; the window touches the image border
        from rsvld_amd import ops
        g = torch.Generator(device=dev).manual_seed(5)
        B, Cc, H, W, th, tw = 2, 4, 40, 56, 24, 32
        yy, xx = (H - th if y0 < 0 else y0), (W - tw if x0 < 0 else x0)
        mask = torch.zeros(B, Cc, H, W, dtype=torch.bool)
        mask[:, :, yy:yy + th, xx:xx + tw] = True
        acc, cnt = _r(g, dev, (B, Cc, H, W)), torch.rand(B, Cc, H, W, generator=g, device=dev)
        tile, wts = _r(g, dev, (B, Cc, th, tw)), torch.rand(th, tw, generator=g, device=dev) + 0.1
        fn = lambda acc, cnt, tile, wts: ops.tile_blend_accumulate(acc, cnt, tile, wts, yy, xx)
        return dict(fn=fn, operands=dict(acc=G.Op(acc, inplace=mask), cnt=G.Op(cnt, inplace=mask), tile=tile, wts=wts))


_tile_blend("top_left_corner", 0, 0)
_tile_blend("bottom_right_corner", -1, -1)       # flush with the last row and column: the last store is the last element of acc
_tile_blend("interior", 3, 5)


@_small("tile_blend_finish", ("tile_blend_finish",))
def _s_blend_finish(dev, dt):
    from rsvld_amd import ops
    g = torch.Generator(device=dev).manual_seed(6)
    return dict(fn=lambda acc, cnt: ops.tile_blend_finish(acc, cnt), operands=dict(acc=_r(g, dev, (2, 4, 40, 57)), cnt=torch.rand(2, 4, 40, 57, generator=g, device=dev) + 0.1))


def _wavelet(shape, radius):
    @_small(f"wavelet_blur_{'x'.join(map(str, shape))}_r{radius}", ("wavelet_blur",))
    def build(dev, dt):      # radius >= H or W: every tap but the centre is clamped to the border ("clamped dilations"); high_accum in place
        from rsvld_amd import ops
        g = torch.Generator(device=dev).manual_seed(shape[-1])
        img, high = torch.rand(shape, generator=g, device=dev) * 2 - 0.5, _r(g, dev, shape)
        return dict(fn=lambda img, high: ops.wavelet_blur(img, radius, high_accum=high), operands=dict(img=img, high=G.Op(high, inplace=True)))


_wavelet((2, 2, 33, 17), 16)     # radius < H, radius ~ W
_wavelet((2, 2, 33, 17), 64)     # radius >= H and W
_wavelet((1, 1, 1, 513), 16)     # H = 1, W > 256
_wavelet((1, 3, 9, 300), 1)


def _adain(shape):
    @_small(f"adain_{'x'.join(map(str, shape))}", ("adain",))
    def build(dev, dt):      # HW = 2 / 323: planes shorter than a workgroup, the statistics workspace guarded
        from rsvld_amd import ops
        g = torch.Generator(device=dev).manual_seed(shape[2])
        return dict(fn=lambda c, s: ops.adain(c, s), operands=dict(c=_r(g, dev, shape) * 2 + 1, s=_r(g, dev, shape) * 0.5 - 3))


_adain((1, 4, 1, 2))
_adain((2, 3, 17, 19))
_adain((1, 2, 64, 64))


@_small("sinusoidal", ("sinusoidal",))
def _s_sin(dev, dt):
    from rsvld_amd import ops
    return dict(fn=lambda lv, t: (ops.sinusoidal(lv, 64, 0), ops.sinusoidal(t, 320, 1)),
                operands=dict(lv=torch.tensor([0.1, 0.7, 0.999], device=dev), t=torch.tensor([0.0, 19.0, 999.0], device=dev)))


@_small("to_planes_as_f32_round_trip", ("to_planes", "as_f32", "maybe_planes"))
def _s_planes(dev, dt):      # 37 x 5 rows of 72 channels: rsvld_split_planes / rsvld_merge_planes at a channel count that is a multiple of 8 only
    from rsvld_amd import ops
    g = _gen(1)
    x = (torch.randn(37, 5, 72, generator=g) * torch.logspace(-6, 4, 72)).to(dev)
    pl = ops.to_planes(torch.randn(2, 9, 11, 40, generator=g).to(dev))
    def fn(x, pl):
        with ops.f32_split(ops.ALL_SPLIT):
            mp = ops.maybe_planes(x)
        assert isinstance(mp, ops.Planes)
        return ops.to_planes(x), ops.as_f32(pl), mp
    return dict(fn=fn, operands=dict(x=x, pl=pl), expect=("split_planes",))


def _q8_finite(name, t):
    """Element test of a Q8Rows tensor ``[..., 2, C]`` (fp16-typed): plane 0 is fp16(x); plane 1 holds e4m3 bytes, of which 0x7F / 0xFF
    are the NaN codes (include/rsvld_hip.h, RSVLD_F16Q8) -- read as fp16 a pair of valid e4m3 bytes may well be an Inf / NaN pattern."""
    if not (name.endswith(".t") and t.dtype == F16 and t.dim() >= 2 and t.shape[-2] == 2):
        return None
    b = t[..., 1, :].contiguous().view(torch.uint8)
    okb = (b & 0x7F) != 0x7F
    return torch.stack([torch.isfinite(t[..., 0, :]), okb[..., 0::2] & okb[..., 1::2]], -2)


@_small("to_q8rows", ("to_q8rows",))
def _s_q8rows(dev, dt):
    from rsvld_amd import ops
    x = (torch.randn(5, 7, 64, generator=_gen(4)) * torch.logspace(-5, 1.5, 64)).to(dev)
    return dict(fn=lambda x: ops.to_q8rows(x), operands=dict(x=x), expect="split_q8", finite=_q8_finite)


# ============================================================================= the tests: one per kernel family
def _params(family):
    return [pytest.param(c, id=c.id) for c in FAMILIES[family]]


@pytest.mark.parametrize("c", _params("conv_igemm"))
def test_guarded_conv_igemm(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("conv_halo"))
def test_guarded_conv_halo(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("gemm256"))
def test_guarded_gemm256(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("attention"))
def test_guarded_attention(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("norms"))
def test_guarded_norms(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("f32_family"))
def test_guarded_f32_family(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("decode"))
def test_guarded_decode(cuda, c):
    _run(cuda, c)


@pytest.mark.parametrize("c", _params("small"))
def test_guarded_small(cuda, c):
    _run(cuda, c)

