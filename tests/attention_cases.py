"""Exact and adversarial inputs for the nine non-causal attention kernels of the diffusion and VAE path -- attn_d64b (4 and 8
waves), attn_d64c, attn_d512b + attn_combine_kernel, attn_d512d (csrc/attention.hip), attn_f32_kernel<false> / <true> (csrc/f32.hip),
attn_split_d64_kernel, attn_split_d512_kernel and the GEMM form around softmax_rows_split_kernel (csrc/split.hip): the input
builders, the fp64 evaluator, the assertions, the fault list and the shape lists behind tests/test_gpu_attention_exact.py, walked
without a GPU by tests/test_attention_cases.py.  The pattern is that of tests/caption_attention_cases.py.

Why: ``randn . randn * D^-0.5`` scores spread a row's weight over every key, so ONE wrong key -- dropped, read twice, read from a
stale LDS buffer, a pad slot admitted -- moves the output by about 1 / Nk of its size and hides under a tolerance taken over the
whole tensor.  Three families; every operand is exactly representable in fp16 AND bf16 (so one set of operands serves every
route: 16-bit, fp32 and planes); a "row" is one (batch b, head h, query index r) triple; tile = 64 keys at D = 64, else 32:

  A  needle    keys are +-1 sign vectors, the query of a row is a x ONE target key (a = 8 / 4 / 2 at D = 64 / 128 / 512: the target
               scores a sqrt(D) = 64 / 45 / 45 nats, every other key a x a sign correlation), V rows are signed integers 1 .. 8 (keys =
               values: the sign vectors themselves): the row's result IS the target's V row to one spacing of the output format,
               a wrong key is off by 1 or more -- provided the other keys' weights x 8 sum to less than 2^-26 (``needle_leak``, fp64).
               The target of row (b, h, r) is slot (b + h + r) mod 8 of NEEDLE_SLOTS; two of the eight are a hash, so that every
               in-tile offset is reached.
  B  counting  q = 0, so every weight is exactly 1 in any arithmetic; V[j] is the unit vector of channel (j + 7 h + 3 b) mod D (the
               shifts make exchanged heads and batches visible): element d of the result is c_d / Nk, c_d = the number of keys whose
               V row is the unit vector of d.  round(got Nk) == c_d, and |got - c_d / Nk| within one spacing.  Keys are random.
  C  ramp      K[j] = sigma x (a nested mask of n_j ones), q = a sigma with a cycling over RAMP_A[D] by (h + r) mod 4 -- over the heads,
               and over the query rows too, so that the single-head routes see +-a as well: unscaled scores a n_j are integers, scaled
               they span 0 .. 32 (D = 64) / 45 nats ascending and descending.  "up": n_j = round(D j / (Nk - 1)), the maximum rises
               (a > 0) or falls (a < 0) over the keys; "saw": n_j runs over 0 .. D inside every tile.  V is random (keys = values: V = K).
               Reference: an fp64 softmax; bound PER ROW max_d |got - want| <= tol max_d sum_j p_j |v_jd| -- the absolute-value
               attention, from the reference alone: cancellation in a row neither loosens nor tightens it.  tol is the suite's own
               constant of the route (TOL16 = _tol of tests/test_gpu_kernels.py, TOL_F32, TOL_SPLIT).

"Random" operands are randn rounded to the grid 2^-6 Z inside (-4, 4): eight significant bits, exact in both 16-bit types.

``reference(case, fault=..., model=..., kps=...)`` evaluates the attention in fp64 with one of FAULTS built in (the CPU test shows
that every fault is rejected by the assertions, i.e. that they would fail on a subtly wrong kernel), or with one of MODELS: a
rounding a kernel's code performs that the plain fp64 softmax does not, for a route whose ramp error is that rounding."""
import functools
import math
import types

import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
DTN = {F16: "f16", BF16: "bf16"}
FMT16 = {F16: "f16", BF16: "bf16"}
TOL16 = {"f16": 4e-3, "bf16": 3e-2}            # _tol of tests/test_gpu_kernels.py
TOL_F32 = 2e-5                                 # REL of tests/test_gpu_f32.py
TOL_SPLIT = 1e-4                               # REL of tests/test_gpu_split.py, REL_SPLIT of tests/test_gpu_f32.py
LEAK_BOUND = 2.0 ** -26
NEEDLE_A = {64: 8.0, 128: 4.0, 512: 2.0}
RAMP_A = {64: (4.0, -4.0, 2.0, -2.0), 128: (4.0, -4.0, 2.0, -2.0), 512: (2.0, -2.0, 1.0, -1.0)}
RAMP_PROFILES = ("up", "saw")
NEEDLE_SLOTS = ("0", "Nk - 1", "first key of the last tile", "the key before it", "tile - 1", "tile", "hash", "hash'")

FAULTS = {
    1: "key `tile` dropped",
    2: "the last key of every full tile dropped",
    3: "the last key counted once more for each pad slot of a ragged tile",
    4: "key Nk // 2 counted twice",
    5: "V rows of keys j and j ^ 4 exchanged in the upper half of each tile",
    6: "heads 0 and 1 exchanged",
    7: "batch 1 reading batch 0's keys",
    8: "the partial of key range 1 dropped",
    9: "the running output not rescaled when the maximum rises in key tile 1",
    10: "a pad column of the GEMM form admitted with score 0",
}
MODELS = {
    "qsplit": "q x fp32(scale log2 e) rounded to fp32 and re-split to a bf16 pair (hi + lo, 16 bits) before the score product: "
              "attn_split_d64_kernel / attn_split_d512_kernel",
}


def tile_of(D):
    return 64 if D == 64 else 32


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes: the smallest at which the code paths differ
# ---------------------------------------------------------------------------------------------------------------------------------
# 16-bit D = 64, (B, heads, Nq, Nk): one to five key tiles (attn_d64c requests three in its prologue and rings four), full and ragged
# last tiles, Nq on both sides of 128 and 512 rows; Nk = 128 / 129 / 191 / 192: both sides of attn_split_d64_kernel's steady / general switch
D64_SHAPES = [(1, 2, 130, 1), (1, 2, 70, 63), (1, 3, 129, 64), (1, 2, 100, 65), (2, 2, 513, 129), (1, 2, 300, 192), (1, 1, 257, 191),
              (1, 2, 140, 250), (1, 2, 600, 273), (1, 1, 300, 333)]
D64_SPLIT_EXTRA = [(1, 1, 40, 128)]            # attn_split_d64_kernel only: exactly two full tiles (the last steady iteration's successor is full)
D64_NW8_SHAPE = (1, 1, 16384, 77)              # un-forced: attn_d64b, 8 waves; needle and counting only
# 16-bit D = 512, (B, Nq, Nk) -> key ranges of attn_d512b's split-KV plan; the same shapes with keys = values
D512_SHAPES = {(1, 1, 1): 1, (1, 33, 31): 1, (1, 130, 32): 1, (1, 100, 33): 1, (2, 144, 95): 1, (1, 100, 333): 1, (1, 64, 600): 2,
               (1, 128, 1024): 4, (1, 300, 2500): 9}
# fp32 kernels, (B, heads, Nq, Nk, D, fused): D = 64 x 2 heads, 128, 512; B = 2 once, q | k | v slices of one tensor once
F32_NQNK = [(33, 1), (45, 31), (32, 32), (70, 33), (100, 77), (40, 333)]
F32_SHAPES = [(1, heads, Nq, Nk, D, False) for heads, D in ((2, 64), (1, 128), (1, 512)) for Nq, Nk in F32_NQNK] + \
             [(2, 2, 70, 33, 64, False), (1, 1, 130, 130, 128, True)]
SPLIT_D512_SHAPES = [(1, 1, 1), (1, 65, 31), (1, 64, 32), (2, 100, 33), (1, 130, 95), (1, 70, 333)]
# GEMM form: pad columns 0 .. 7 and a second 2048-column pass of softmax_rows_split_kernel; Nq = 300 = two row blocks of 256
GEMM_NQ, GEMM_NK, GEMM_D = 300, [1, 7, 8, 9, 333, 2049, 2500], (512, 128)


# ---------------------------------------------------------------------------------------------------------------------------------
# case objects: family, label, shape = (B, heads, Nq, Nk, D), tile, scale, shared (keys = values), q64 [B, heads, Nq, D],
#               k64 / v64 [B, heads, Nk, D] (fp64); needle: targets [B, heads, Nq], want [B, heads, Nq, D]; counting: counts [B, heads, D]
# ---------------------------------------------------------------------------------------------------------------------------------
def _signs(shape, gen):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()


def _grid(shape, gen):
    """randn on the grid 2^-6 Z, |x| <= 4 - 2^-6: at most eight significant bits."""
    return (torch.round(torch.randn(shape, generator=gen, dtype=torch.float64) * 64) / 64).clamp(-4 + 2.0 ** -6, 4 - 2.0 ** -6)


def _case(family, label, shape, shared, q64, k64, v64, **extra):
    B, heads, Nq, Nk, D = shape
    assert q64.shape == (B, heads, Nq, D) and k64.shape == (B, heads, Nk, D) and v64.shape == k64.shape
    return types.SimpleNamespace(family=family, label=f"{shape}{' k=v' if shared else ''} {label}", shape=shape, B=B, heads=heads, Nq=Nq, Nk=Nk,
                                 D=D, tile=tile_of(D), scale=D ** -0.5, shared=shared, q64=q64, k64=k64, v64=v64, _ref=None, **extra)


def representable(c):
    """Every operand survives a round trip through fp16 and through bf16."""
    return all(torch.equal(x.to(dt).double(), x) for x in (c.q64, c.k64, c.v64) for dt in DTYPES)


def needle_target(b, h, r, Nk, tile):
    slot = (b + h + r) % 8
    last = tile * ((Nk - 1) // tile)
    if slot >= 6:
        return ((((b * 65536 + r) * 16 + h) * 2 + slot - 5) * 2654435761 >> 9) % Nk
    return min(max((0, Nk - 1, last, last - 1, tile - 1, tile)[slot], 0), Nk - 1)


@functools.lru_cache(maxsize=None)
def needle(shape, shared=False):
    B, heads, Nq, Nk, D = shape
    gen = torch.Generator().manual_seed(11 + 1000 * Nq + Nk + D + 7 * heads + shared)
    ks = _signs((B, heads, Nk, D), gen)
    v = ks if shared else _signs((B, heads, Nk, D), gen) * torch.randint(1, 9, (B, heads, Nk, D), generator=gen).double()
    tg = torch.tensor([[[needle_target(b, h, r, Nk, tile_of(D)) for r in range(Nq)] for h in range(heads)] for b in range(B)])
    idx = tg[..., None].expand(B, heads, Nq, D)
    return _case("needle", "needle", shape, shared, NEEDLE_A[D] * torch.gather(ks, 2, idx), ks, v, targets=tg, want=torch.gather(v, 2, idx))


def needle_leak(c):
    """Per row [B, heads, Nq], fp64: 8 x the weight of every key but the target, relative to the target's."""
    s = _scores(c.q64, c.k64, c.scale)
    tgt = c.targets[..., None]
    d = torch.exp(s - s.gather(-1, tgt))
    d.scatter_(-1, tgt, 0.0)
    return 8.0 * d.sum(-1)


def distinct_rows(x):
    """No two rows of any [.., N, D] slice of x are equal."""
    return all(len(torch.unique(m, dim=0)) == m.shape[0] for m in x.reshape(-1, x.shape[-2], x.shape[-1]))


@functools.lru_cache(maxsize=None)
def counting(shape, shared=False):
    B, heads, Nq, Nk, D = shape
    gen = torch.Generator().manual_seed(21 + 1000 * Nq + Nk + D + 7 * heads + shared)
    b, h, j = torch.meshgrid(torch.arange(B), torch.arange(heads), torch.arange(Nk), indexing="ij")
    v = torch.zeros(B, heads, Nk, D, dtype=torch.float64)
    v[b, h, j, (j + 7 * h + 3 * b) % D] = 1.0
    k = v if shared else _grid((B, heads, Nk, D), gen)
    return _case("counting", "counting", shape, shared, torch.zeros(B, heads, Nq, D, dtype=torch.float64), k, v, counts=v.sum(dim=2))


def ramp_counts(profile, Nk, D):
    """n_j [Nk]: the number of ones in the mask of key j."""
    j = torch.arange(Nk, dtype=torch.float64)
    if profile == "saw" and Nk > 1:
        tile = tile_of(D)
        return torch.round(D * (j % tile) / (tile - 1)).long()
    return torch.full((1,), D) if Nk == 1 else torch.round(D * j / (Nk - 1)).long()


@functools.lru_cache(maxsize=None)
def ramp(shape, profile, shared=False):
    B, heads, Nq, Nk, D = shape
    gen = torch.Generator().manual_seed(31 + 1000 * Nq + Nk + D + 7 * heads + shared + 2 * (profile == "saw"))
    sigma = _signs((B, heads, D), gen)
    rank = torch.rand(B, heads, D, generator=gen).argsort(dim=-1).argsort(dim=-1)    # nested masks: channel d is in mask j iff rank[d] < n_j
    nj = ramp_counts(profile, Nk, D)
    k = sigma[:, :, None, :] * (rank[:, :, None, :] < nj[None, None, :, None]).double()
    a = torch.tensor([[RAMP_A[D][(h + r) % 4] for r in range(Nq)] for h in range(heads)], dtype=torch.float64)      # [heads, Nq]
    q = a[None, :, :, None] * sigma[:, :, None, :]
    v = k if shared else _grid((B, heads, Nk, D), gen)
    return _case("ramp", f"ramp/{profile}", shape, shared, q, k, v, profile=profile, a=a, nj=nj)


def ramp_scores_exact(c):
    """The fp64 q . k of a ramp case IS a n_j: integers below 2^11, exact in any fp32 accumulation order."""
    s = torch.einsum("bhqd,bhkd->bhqk", c.q64, c.k64)
    want = c.a[None, :, :, None] * c.nj[None, None, None, :].double()
    return torch.equal(s, want.expand_as(s)) and float(s.abs().max()) < 2048


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 evaluator
# ---------------------------------------------------------------------------------------------------------------------------------
def _scores(q64, k64, scale):
    return torch.einsum("bhqd,bhkd->bhqk", q64, k64) * scale


def _qsplit(q64, scale):
    """MODELS["qsplit"]: what the split kernels contract with K, in units of nats per unit of k (csrc/split.hip: f = (hi + lo) *
    scale_log2e in fp32, qh = bf16(f), ql = bf16(f - qh); scale_log2e = scale * 1.44269504088896340736f in fp32)."""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    f = q64.float() * c
    hi = f.bfloat16().float()
    lo = (f - hi).bfloat16().float()
    return (hi.double() + lo.double()) * math.log(2.0)


def reference(c, fault=None, model=None, kps=0):
    """softmax(q K^T scale) V in fp64 -> [B, heads, Nq, D].  ``fault``: a key of FAULTS, built in; ``model``: a key of MODELS;
    ``kps``: keys per range of the route's split-KV plan (fault 8; 0: no split)."""
    assert fault is None or fault in FAULTS
    assert model is None or model in MODELS
    if fault is None and model is None and c._ref is not None:
        return c._ref
    k64, v64, Nk, tile = c.k64, c.v64, c.Nk, c.tile
    keys = torch.arange(Nk)
    if fault == 7 and c.B >= 2:
        k64 = k64.clone()
        k64[1] = k64[0]
        if c.shared:
            v64 = k64
    if fault == 5:
        src = torch.where((keys % tile >= tile // 2) & ((keys ^ 4) < Nk), keys ^ 4, keys)
        v64 = v64[:, :, src]
    mult = torch.ones(Nk, dtype=torch.float64)                        # how often every row counts a key
    if fault == 1 and Nk > tile:
        mult[tile] = 0.0
    if fault == 2:
        mult[keys % tile == tile - 1] = 0.0
    if fault == 3:
        mult[Nk - 1] += (-Nk) % tile
    if fault == 4:
        mult[Nk // 2] = 2.0
    if fault == 8 and kps:
        mult[kps:2 * kps] = 0.0
    s = _scores(c.q64, k64, c.scale) if model is None else torch.einsum("bhqd,bhkd->bhqk", _qsplit(c.q64, c.scale), k64)
    s = s.masked_fill(mult == 0, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    if fault == 10 and Nk % 8:
        m = m.clamp(min=0.0)
    w = torch.exp(s - m) * mult
    den = w.sum(dim=-1, keepdim=True)
    if fault == 10 and Nk % 8:
        den = den + torch.exp(-m)                                      # one pad column: score 0, a zero V row
    num = w
    if fault == 9 and Nk > tile:
        m0 = s[..., :tile].max(dim=-1, keepdim=True).values
        m1 = torch.maximum(m0, s[..., tile:2 * tile].max(dim=-1, keepdim=True).values)
        num = w.clone()
        num[..., :tile] *= torch.exp(m1 - m0)                          # tile 0's sum kept at its own maximum: the factor exp(m0 - m1) missing
    out = torch.einsum("bhqk,bhkd->bhqd", num, v64) / den
    if fault == 6 and c.heads >= 2:
        out = out[:, [1, 0] + list(range(2, c.heads))]
    if fault is None and model is None:
        c._ref = out
        c._scale = torch.einsum("bhqk,bhkd->bhqd", w / den, v64.abs()).amax(dim=-1)     # max_d sum_j p_j |v_jd| per row
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the assertions (the GPU test applies them to the kernels' output, the CPU test to ``reference`` with and without a fault)
# ---------------------------------------------------------------------------------------------------------------------------------
FMTS = ("f16", "bf16", "planes", "f32")


def round_to(x64, fmt):
    """One rounding of an fp64 tensor to an output format: a 16-bit type, fp32, or planes (fp32 -> bf16 hi + bf16 lo)."""
    if fmt in ("f16", "bf16"):
        return x64.to(F16 if fmt == "f16" else BF16).double()
    x = x64.float()
    if fmt == "f32":
        return x.double()
    hi = x.bfloat16().float()
    return hi.double() + (x - hi).bfloat16().double()


def spacing(want, fmt):
    """The assertion's unit at ``want`` (fp64): the spacing of the 16-bit type; 2^-16 relative for planes; 8 x 2^-24 relative for fp32."""
    if fmt in ("f16", "bf16"):
        from test_gpu_gemv_mma import _ulp
        return _ulp(want, F16 if fmt == "f16" else BF16)
    return want.abs() * (2.0 ** -16 if fmt == "planes" else 8 * 2.0 ** -24)


def unpack(c, got):
    """The result of a call, [B, Nq, heads D] on any device, in any float type -> fp64 [B, heads, Nq, D] on the host."""
    return got.detach().cpu().double().reshape(c.B, c.Nq, c.heads, c.D).transpose(1, 2)


def pack(x64):
    """[B, heads, N, D] -> [B, N, heads D], the layout of ops.attention."""
    B, heads, N, D = x64.shape
    return x64.transpose(1, 2).reshape(B, N, heads * D)


def ramp_ratio(c, got, tol, model=None):
    """Per row [B, heads, Nq]: max_d |got - want| / (tol max_d sum_j p_j |v_jd|), the error and the bound.  ``want``: the plain fp64
    softmax, or the modelled one; the bound's scale is always that of the plain one."""
    want = reference(c, model=model)
    reference(c)
    err, bound = (got - want).abs().amax(dim=-1), tol * c._scale
    return torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err)), err, bound


def check(c, got, fmt, tol=None, model=None):
    """``got``: fp64 [B, heads, Nq, D] in the values of format ``fmt`` (``unpack`` of a kernel's result; ``round_to`` of a reference).
    Raises AssertionError; returns (the worst ratio of an error to its bound, whether a needle's result was bit-equal, else None)."""
    assert fmt in FMTS and got.shape == c.q64.shape and got.dtype == torch.float64
    assert bool(torch.isfinite(got).all()), f"{c.label}: non-finite output"

    def where(bad):
        b, h, r = (int(x) for x in bad.nonzero()[0])
        return f"{int(bad.sum())} rows, first: batch {b} head {h} query {r}"
    if c.family == "needle":
        err, bound = (got - c.want).abs(), spacing(c.want, fmt)
        bad = (err > bound).any(dim=-1)
        if bool(bad.any()):
            b, h, r = (int(x) for x in bad.nonzero()[0])
            raise AssertionError(f"{c.label} [{fmt}]: {where(bad)} (target key {int(c.targets[b, h, r])}) differ from their target's V row, "
                                 f"max|d| = {float(err[b, h, r].max()):.3g}")
        return float((err / bound).max()), torch.equal(got, c.want)
    if c.family == "counting":
        cd = c.counts[:, :, None, :].expand_as(got)
        want = cd / c.Nk
        err, bound = (got - want).abs(), spacing(want, fmt)
        bad = (err > bound).any(dim=-1)
        assert not bool(bad.any()), f"{c.label} [{fmt}]: {where(bad)} off c_d / Nk by more than one spacing"
        bad = (torch.round(got * c.Nk) != cd).any(dim=-1)
        assert not bool(bad.any()), f"{c.label} [{fmt}]: {where(bad)}: a key was not counted once"
        return float(torch.where(bound > 0, err / bound, err).max()), None
    ratio, err, bound = ramp_ratio(c, got, tol, model)
    worst = float(ratio.max())
    if worst > 1.0:
        b, h, r = (int(x) for x in (ratio > 1.0).nonzero()[0])
        raise AssertionError(f"{c.label} [{fmt}{', model ' + model if model else ''}]: {where(ratio > 1.0)}: max_d|d| = {float(err[b, h, r]):.3e} > "
                             f"{float(bound[b, h, r]):.3e} (worst ratio {worst:.3g})")
    return worst, None


# ---------------------------------------------------------------------------------------------------------------------------------
# the routes: name -> what runs, on which shapes, judged how.  ``shapes``: (B, heads, Nq, Nk, D) tuples; ``fmt``: None = the two
# 16-bit types; ``kps(shape)``: keys per range of the route's split-KV plan, asked of the planner by the CPU test (0: one range).
# ---------------------------------------------------------------------------------------------------------------------------------
def _d64(shapes):
    return [s + (64,) for s in shapes]


def _d512(shapes):
    return [(B, 1, Nq, Nk, 512) for B, Nq, Nk in shapes]


ROUTES = {
    "d64": dict(shapes=_d64(D64_SHAPES), shared=False, fmt=None, tol=TOL16),
    "d64_nw8": dict(shapes=_d64([D64_NW8_SHAPE]), shared=False, fmt=None, tol=TOL16, families=("needle", "counting")),
    "d512b": dict(shapes=_d512(D512_SHAPES), shared=False, fmt=None, tol=TOL16),
    "d512d": dict(shapes=_d512(D512_SHAPES), shared=True, fmt=None, tol=TOL16),
    "d512b_shared": dict(shapes=_d512(D512_SHAPES), shared=True, fmt=None, tol=TOL16),
    "f32": dict(shapes=[s[:5] for s in F32_SHAPES], shared=False, fmt="f32", tol=TOL_F32),
    "f32_split": dict(shapes=[s[:5] for s in F32_SHAPES], shared=False, fmt="f32", tol=TOL_SPLIT),
    "split_d64": dict(shapes=_d64(D64_SHAPES + D64_SPLIT_EXTRA), shared=False, fmt="planes", tol=TOL_SPLIT),
    "split_d512": dict(shapes=_d512(SPLIT_D512_SHAPES), shared=True, fmt="planes", tol=TOL_SPLIT),
    "gemm": dict(shapes=[(1, 1, GEMM_NQ, Nk, D) for D in GEMM_D for Nk in GEMM_NK], shared=False, fmt="planes", tol=TOL_SPLIT),
}
# A ramp bound that a route meets only against a modelled reference: {route: key of MODELS} (tests/test_gpu_attention_exact.py says why)
ROUTE_MODEL = {}
FAMILIES = ("needle", "counting", "ramp")


def route_fmts(route):
    return ("f16", "bf16") if ROUTES[route]["fmt"] is None else (ROUTES[route]["fmt"],)


def route_tol(route, fmt):
    tol = ROUTES[route]["tol"]
    return tol[fmt] if isinstance(tol, dict) else tol


def cases(shape, shared=False, families=FAMILIES):
    if "needle" in families:
        yield needle(shape, shared)
    if "counting" in families:
        yield counting(shape, shared)
    if "ramp" in families:
        for profile in RAMP_PROFILES:
            yield ramp(shape, profile, shared)


def route_cases(route, shape=None):
    r = ROUTES[route]
    for s in r["shapes"] if shape is None else [shape]:
        yield from cases(s, r["shared"], r.get("families", FAMILIES))
