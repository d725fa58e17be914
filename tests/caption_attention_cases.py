"""Exact and adversarial inputs for the caption's two softmax attentions -- the decode step (da_kernel + da_combine_kernel of
csrc/decode_attention.hip, through ops.llama_decode_attention / decode_rows.llama_decode_attention_rows) and the flash prefill
(prefill_attn_d128_kernel of csrc/prefill_attention.hip): the input builders, the fp64 references, the assertions and the
preconditions behind tests/test_gpu_caption_attention.py, walked without a GPU by tests/test_caption_attention_cases.py.

Why: ``randn . randn / sqrt(128)`` scores stay in [-4, 4] and spread a row's weight over every key, so a fault in ONE key changes
the output by about 1 / (number of keys) and hides under a tolerance taken over the whole output.  Three families, every operand
exactly representable in fp16 AND bf16, head_dim 128, scale 128^-0.5; a "row" is one (position p, query head h) pair:

  A  needle    keys are sign vectors, the (rotated) query of a row is 4 x ONE target key c <= p: the target scores 512 (45.3
               scaled), every other key 4 x a sign correlation, so the row's result IS the target's integer-valued V row --
               ``torch.equal``, no tolerance -- provided the other keys' weights sum to less than 2^-12 / 8 (``needle_leak``,
               computed in fp64).  The target of row (t, h) is family (t + h) mod 8 of NEEDLE_FAMILIES ("table"), or a hash of
               (p, h) ("scatter": the eight families reach only the in-tile offsets 0 and 39..63 BELOW a row's own key tile, since
               (37 p + 11) mod (p + 1) = p - 25 from p = 26 on; the hashed targets reach all 64).
  B  counting  q = 0, so every weight is exactly 1 in any arithmetic; V[j] is the unit vector of channel j mod 128: element d of
               the result is (number of keys j <= p congruent to d) / (p + 1) -- every row visited every key up to its position
               exactly once.  One spacing of T covers the rounding to T and the fp32 reciprocal.
  C  ramp      K[j] = sigma x (a mask of n_j ones), q = a_h sigma with a_h cycling over (4, -4, 2, -2): unscaled scores a_h n_j are
               integers exact in bf16, scaled they span 0 .. 45 ascending and descending over one cache.  "up": n_j = round(128 j /
               (n - 1)), the maximum rises by several units per key tile and early chunks underflow in the combine; "saw": n_j =
               2 (j mod 64), every tile spans the whole range.  V = randn rounded to T, the reference an fp64 softmax, the bound
               the project's 4e-3 / 3e-2 (test_gpu_kernels._close) PER ROW: max_d |got - want| <= tol max_d |want_row|.

The decode kernel applies the rotary embedding itself: the builders draw a quarter turn per frequency (cos, sin in {0, +1, -1},
duplicated over both halves as FastDecoder passes them) and hand the kernel the exact pre-image of the q and k they want after the
rotation -- a signed permutation, so T(x cos) + T(rot(x) sin) is exact.  The cache of a decode case holds a stale row at ``pos``
that differs from the new key and value, and decoys in every slot above ``pos`` (prefill: above the call's last position): one
admitted slot moves every element of the result.

``reference(case, fault=...)`` evaluates the attention in fp64 with one of FAULTS built in: the CPU test shows that every fault
is rejected by the assertions above, i.e. that they would fail on a subtly wrong kernel."""
import functools
import types

import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
DTN = {F16: "f16", BF16: "bf16"}
HD = 128
SCALE = HD ** -0.5
TOL = {F16: 4e-3, BF16: 3e-2}                  # _close of tests/test_gpu_kernels.py
LEAK_BOUND = 2.0 ** -12

# ---------------------------------------------------------------------------------------------------------------------------------
# shapes: the smallest at which the code paths differ
# ---------------------------------------------------------------------------------------------------------------------------------
# prefill (T, pos0, n_q, n_kv, max_len): the two of tests/test_gpu_prefill_attention.py every family runs on, and the group sizes
# g = 2, 3, 6, 5, 6, 7 (128 rows per workgroup and 32 per wave are no multiple of 3, 5, 6, 7: a token's heads straddle waves)
PREFILL_BASE = [(300, 0, 8, 2, 384), (60, 100, 8, 2, 192)]
PREFILL_GROUPS = [(130, 0, 2, 1, 192), (45, 0, 3, 1, 64), (70, 30, 6, 2, 128), (30, 70, 5, 1, 128), (50, 90, 12, 2, 192), (40, 0, 7, 1, 64)]
# decode (n_q, n_kv): G = 1, 2, 3, 5, 6, 7, 8 (G > 4: a second pass of the per-head loops; G < 4: idle waves) and the suite's G = 4
DECODE_GROUPS = [(4, 4), (4, 2), (3, 1), (5, 1), (12, 2), (7, 1), (8, 1), (8, 2)]
DECODE_RAMP_GROUPS = [(8, 1), (8, 2)]
# (max_len, pos): one key; the last key of chunk 0; one key in chunk 1; mid-chunk; the last slot; a cache shorter than one chunk
DECODE_POSITIONS = [(384, 0), (384, 127), (384, 128), (384, 300), (384, 383), (100, 99)]
# da_combine_kernel's second round (more than 64 chunks): 66 chunks; round two empty, round one full, one key in round two, the last slot
COMBINE_GROUP, COMBINE_MAX_LEN = (2, 1), 8325
COMBINE_POSITIONS = [100, 8191, 8192, 8324]
COMBINE_ROWS = [100, 8192, 8324]               # the same through llama_decode_attention_rows, B = 3
RAMP_PROFILES = ("up", "saw")
RAMP_A = (4, -4, 2, -2)

NEEDLE_FAMILIES = ("p", "0", "p-1", "64 floor(p/64)", "64 floor(p/64) - 1", "128 floor(p/128) - 1", "(37 p + 11) mod (p + 1)", "min(p, 63)")

FAULTS = {
    1: "key 64 dropped for rows p > 64",
    2: "the last key of every full 128-key chunk dropped",
    3: "the stale cache row used for the new token's key (decode)",
    4: "key p // 2 counted twice",
    5: "V rows of keys j and j ^ 4 exchanged in the upper half of each 64-key tile",
    6: "heads 0 and 1 of every group exchanged",
    7: "the partial of the first chunk of the second combine round (keys 8192 .. 8319) dropped",
    8: "the running output not rescaled when the maximum rises in key tile 1",
}


def needle_target(p, t, h, variant="table"):
    """The target key of row (token index t of the call, position p, head h), clamped to [0, p]."""
    if variant == "scatter":
        return ((p * 16 + h + 1) * 2654435761 >> 9) % (p + 1)
    c = (p, 0, p - 1, 64 * (p // 64), 64 * (p // 64) - 1, 128 * (p // 128) - 1, (37 * p + 11) % (p + 1), min(p, 63))[(t + h) % 8]
    return min(max(c, 0), p)


def _exact(x, dtype, what):
    assert torch.equal(x.to(dtype).double(), x), f"{what} is not representable in {DTN[dtype]}"
    return x.to(dtype)


def _signs(shape, gen):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# rotary embedding by quarter turns (decode)
# ---------------------------------------------------------------------------------------------------------------------------------
def rope(x, cos, sin):
    """The half-split rotation as da_kernel forms it, in fp64: x cos + rot(x) sin, rot(x) = (-x[64:], x[:64])."""
    half = HD // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * sin


def _quarter_turns(gen):
    qt = torch.randint(0, 4, (HD // 2,), generator=gen)
    cos, sin = torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=torch.float64)[qt], torch.tensor([0.0, 1.0, 0.0, -1.0], dtype=torch.float64)[qt]
    return torch.cat([cos, cos]), torch.cat([sin, sin])


def _pre_image(want, cos, sin):
    """x with rope(x) = want: the rotation by the opposite angle (exact: a signed permutation)."""
    x = rope(want, cos, -sin)
    assert torch.equal(rope(x, cos, sin), want)
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# case objects
#   every case: kind, family, label, dtype, n_q, n_kv, max_len, positions [R] (python ints), q64 [R, n_q, HD] (after the rotation),
#               k64 / v64 [n_kv, n, HD]: keys 0 .. n - 1 = the last position, as the attention must see them; tile (64 / 128)
#   prefill:    pos0, q [T, n_q, HD], k / v [n_kv, max_len, HD] in dtype
#   decode:     pos, qkv [(n_q + 2 n_kv) HD], cos / sin [HD], kc / vc [n_kv, max_len, HD] BEFORE the call, new_k / new_v [n_kv, HD] (the
#               rows the call must write at pos), stale_k64 [n_kv, HD]
# ---------------------------------------------------------------------------------------------------------------------------------
def _prefill_case(family, label, dtype, shape, q64, k64, v64, above_k, above_v, **extra):
    T, pos0, n_q, n_kv, max_len = shape
    n = pos0 + T
    k = torch.empty(n_kv, max_len, HD, dtype=torch.float64)
    v = torch.empty(n_kv, max_len, HD, dtype=torch.float64)
    k[:, :n], v[:, :n] = k64, v64
    k[:, n:], v[:, n:] = above_k[:, None], above_v
    return types.SimpleNamespace(kind="prefill", family=family, label=f"prefill {shape} {label}", dtype=dtype, n_q=n_q, n_kv=n_kv,
                                 max_len=max_len, pos0=pos0, positions=list(range(pos0, n)), tile=64, q64=q64, k64=k64, v64=v64,
                                 q=_exact(q64, dtype, "q"), k=_exact(k, dtype, "K"), v=_exact(v, dtype, "V"), **extra)


def _decode_case(family, label, dtype, n_q, n_kv, max_len, pos, q64, k64, v64, stale_k, stale_v, above_k, above_v, gen, **extra):
    """q64 [n_q, HD]; k64 / v64 [n_kv, pos + 1, HD] with the new token's row at ``pos``."""
    cos, sin = _quarter_turns(gen)
    new_k, new_v = k64[:, pos].clone(), v64[:, pos].clone()
    assert not torch.equal(stale_k, new_k) and not torch.equal(stale_v, new_v)
    kc = torch.empty(n_kv, max_len, HD, dtype=torch.float64)
    vc = torch.empty(n_kv, max_len, HD, dtype=torch.float64)
    kc[:, :pos + 1], vc[:, :pos + 1] = k64, v64
    kc[:, pos], vc[:, pos] = stale_k, stale_v
    kc[:, pos + 1:], vc[:, pos + 1:] = above_k[:, None], above_v
    qkv = torch.cat([_pre_image(q64, cos, sin), _pre_image(new_k, cos, sin), new_v]).reshape(-1)
    return types.SimpleNamespace(kind="decode", family=family, label=f"decode q{n_q} kv{n_kv} len {max_len} pos {pos} {label}", dtype=dtype,
                                 n_q=n_q, n_kv=n_kv, max_len=max_len, pos=pos, positions=[pos], tile=128, q64=q64[None], k64=k64, v64=v64,
                                 stale_k64=stale_k, qkv=_exact(qkv, dtype, "qkv"), cos=_exact(cos, dtype, "cos"), sin=_exact(sin, dtype, "sin"),
                                 kc=_exact(kc, dtype, "K cache"), vc=_exact(vc, dtype, "V cache"), new_k=_exact(new_k, dtype, "new k"),
                                 new_v=_exact(new_v, dtype, "new v"), **extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# A  needle
# ---------------------------------------------------------------------------------------------------------------------------------
NEEDLE_SEED = 11


def _needle_parts(n_q, n_kv, n, rows, variant, gen):
    """rows: [(t, p)].  -> sign keys [n_kv, n, HD], V, targets [R, n_q], q64 [R, n_q, HD], want [R, n_q, HD], decoy keys [n_kv, HD]."""
    g = n_q // n_kv
    ks = _signs((n_kv, n, HD), gen)
    v = _signs((n_kv, n, HD), gen) * torch.randint(1, 9, (n_kv, n, HD), generator=gen).double()
    tg = torch.tensor([[needle_target(p, t, h, variant) for h in range(n_q)] for t, p in rows])
    kvh = torch.arange(n_q) // g
    q64, want = 4.0 * ks[kvh[None, :], tg], v[kvh[None, :], tg]
    decoy = 8.0 * ks[torch.arange(n_kv), tg[-1, ::g]]             # the target of the last row's first head of every group
    return ks, v, tg, q64, want, decoy


@functools.lru_cache(maxsize=None)
def needle_prefill(shape, dtype, variant="table"):
    T, pos0, n_q, n_kv, max_len = shape
    gen = torch.Generator().manual_seed(NEEDLE_SEED + 1000 * T + pos0 + n_q)
    ks, v, tg, q64, want, decoy = _needle_parts(n_q, n_kv, pos0 + T, [(t, pos0 + t) for t in range(T)], variant, gen)
    return _prefill_case("needle", f"needle/{variant}", dtype, shape, q64, ks, v, decoy, 100.0, targets=tg, want=want)


@functools.lru_cache(maxsize=None)
def needle_decode(n_q, n_kv, max_len, pos, t, dtype):
    """``t``: the index of ``pos`` in its position list, so that every family occurs over the positions of a group."""
    gen = torch.Generator().manual_seed(NEEDLE_SEED + 100000 * n_q + 1000 * n_kv + pos)
    ks, v, tg, q64, want, decoy = _needle_parts(n_q, n_kv, pos + 1, [(t, pos)], "table", gen)
    stale_k = _signs((n_kv, HD), gen)
    stale_v = _signs((n_kv, HD), gen) * torch.randint(1, 9, (n_kv, HD), generator=gen).double()
    return _decode_case("needle", "needle", dtype, n_q, n_kv, max_len, pos, q64[0], ks, v, stale_k, stale_v, decoy, 100.0, gen,
                        targets=tg, want=want)


def needle_leak(c):
    """Per row [R, n_q], fp64: 8 x the weight of every visible key but the target, relative to the target's."""
    s = _scores(c)
    tgt = c.targets[..., None]
    d = torch.exp(s - s.gather(-1, tgt))
    d.scatter_(-1, tgt, 0.0)
    return 8.0 * d.sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# B  counting
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit_rows(n_kv, n):
    v = torch.zeros(n_kv, n, HD, dtype=torch.float64)
    v[:, torch.arange(n), torch.arange(n) % HD] = 1.0
    return v


def counts(p):
    """c_d [HD] (fp64): the number of keys j <= p with j mod 128 = d."""
    d = torch.arange(HD)
    return torch.where(d <= p, (p - d) // HD + 1, torch.zeros_like(d)).double()


@functools.lru_cache(maxsize=None)
def counting_prefill(shape, dtype):
    T, pos0, n_q, n_kv, max_len = shape
    gen = torch.Generator().manual_seed(21 + 1000 * T + pos0 + n_q)
    n = pos0 + T
    k = torch.randn(n_kv, n, HD, generator=gen).to(dtype).double()
    above_k = torch.randn(n_kv, HD, generator=gen).to(dtype).double()
    return _prefill_case("counting", "counting", dtype, shape, torch.zeros(T, n_q, HD, dtype=torch.float64), k, _unit_rows(n_kv, n),
                         above_k, 100.0)


@functools.lru_cache(maxsize=None)
def counting_decode(n_q, n_kv, max_len, pos, dtype):
    gen = torch.Generator().manual_seed(22 + 100000 * n_q + 1000 * n_kv + pos)
    k = torch.randn(n_kv, pos + 1, HD, generator=gen).to(dtype).double()
    stale_k, above_k = (torch.randn(n_kv, HD, generator=gen).to(dtype).double() for _ in range(2))
    return _decode_case("counting", "counting", dtype, n_q, n_kv, max_len, pos, torch.zeros(n_q, HD, dtype=torch.float64), k,
                        _unit_rows(n_kv, pos + 1), stale_k, torch.full((n_kv, HD), 3.0, dtype=torch.float64), above_k, 100.0, gen)


# ---------------------------------------------------------------------------------------------------------------------------------
# C  ramp
# ---------------------------------------------------------------------------------------------------------------------------------
def ramp_counts(profile, n):
    """n_j [n]: the number of ones in the mask of key j."""
    j = torch.arange(n)
    if profile == "saw":
        return 2 * (j % 64)
    return torch.full((1,), HD) if n == 1 else torch.round(HD * j.double() / (n - 1)).long()


def _ramp_parts(profile, dtype, n_q, n_kv, n, gen):
    g = n_q // n_kv
    sigma = _signs((n_kv, HD), gen)
    rank = torch.rand(n_kv, HD, generator=gen).argsort(dim=1).argsort(dim=1)                        # nested masks: channel d is in mask j iff rank[d] < n_j
    nj = ramp_counts(profile, n)
    k = sigma[:, None, :] * (rank[:, None, :] < nj[None, :, None]).double()
    a = torch.tensor([RAMP_A[(h % g) % 4] for h in range(n_q)], dtype=torch.float64)
    q = a[:, None] * sigma.repeat_interleave(g, dim=0)
    s = a[:, None] * nj[None, :].double()                                                           # the unscaled scores, [n_q, n]
    assert torch.equal(s.to(dtype).double(), s), "a ramp score is not representable"
    assert torch.equal(torch.einsum("hd,hkd->hk", q, k.repeat_interleave(g, dim=0)), s)
    v = torch.randn(n_kv, n, HD, generator=gen).to(dtype).double()
    return sigma, q, k, v


@functools.lru_cache(maxsize=None)
def ramp_prefill(shape, dtype, profile):
    T, pos0, n_q, n_kv, max_len = shape
    gen = torch.Generator().manual_seed(31 + 1000 * T + pos0 + n_q + (profile == "saw"))
    sigma, q, k, v = _ramp_parts(profile, dtype, n_q, n_kv, pos0 + T, gen)
    return _prefill_case("ramp", f"ramp/{profile}", dtype, shape, q[None].expand(T, n_q, HD).contiguous(), k, v, 8.0 * sigma, 100.0)


@functools.lru_cache(maxsize=None)
def ramp_decode(n_q, n_kv, max_len, pos, dtype, profile):
    """The ramp ends at ``pos`` (n = pos + 1), so every position sees the whole range of scores."""
    gen = torch.Generator().manual_seed(32 + 100000 * n_q + 1000 * n_kv + pos + (profile == "saw"))
    sigma, q, k, v = _ramp_parts(profile, dtype, n_q, n_kv, pos + 1, gen)
    stale_k = -sigma if float(k[:, pos].abs().sum()) == 0 else torch.zeros(n_kv, HD, dtype=torch.float64)
    stale_v = torch.randn(n_kv, HD, generator=gen).to(dtype).double()
    return _decode_case("ramp", f"ramp/{profile}", dtype, n_q, n_kv, max_len, pos, q, k, v, stale_k, stale_v, 8.0 * sigma, 100.0, gen)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 evaluator
# ---------------------------------------------------------------------------------------------------------------------------------
def _scores(c, k64=None):
    """Scaled scores [R, n_q, n] in fp64, -inf above a row's position."""
    k64 = c.k64 if k64 is None else k64
    g = c.n_q // c.n_kv
    s = torch.einsum("rhd,hkd->rhk", c.q64, k64.repeat_interleave(g, dim=0)) * SCALE
    above = torch.arange(k64.shape[1])[None, :] > torch.tensor(c.positions)[:, None]
    return s.masked_fill(above[:, None, :], float("-inf"))


def reference(c, fault=None):
    """softmax(q K^T scale) V over keys 0 .. p of every row, fp64 -> [R, n_q, HD]; ``fault``: a key of FAULTS, built in."""
    assert fault is None or fault in FAULTS
    g = c.n_q // c.n_kv
    k64, v64 = c.k64, c.v64
    n = k64.shape[1]
    pos, keys = torch.tensor(c.positions)[:, None], torch.arange(n)[None, :]
    if fault == 3 and c.kind == "decode":
        k64 = k64.clone()
        k64[:, c.pos] = c.stale_k64
    if fault == 5:
        src = torch.where((keys[0] % 64 >= 32) & ((keys[0] ^ 4) < n), keys[0] ^ 4, keys[0])
        v64 = v64[:, src]
    mult = torch.ones(len(c.positions), n, dtype=torch.float64)       # how often a row counts a key
    if fault == 1:
        mult[(keys == 64) & (pos > 64)] = 0.0
    if fault == 2:
        mult[(keys % 128 == 127) & (keys <= pos)] = 0.0
    if fault == 4:
        mult[keys == pos // 2] = 2.0
    if fault == 7:
        mult[(keys >= 8192) & (keys < 8320) & (pos >= 8192)] = 0.0
    s = _scores(c, k64)
    s = s.masked_fill((mult == 0)[:, None, :], float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    w = torch.exp(s - m) * mult[:, None, :]
    num = w
    if fault == 8 and n > c.tile:
        m0 = s[..., :c.tile].max(dim=-1, keepdim=True).values
        m1 = torch.maximum(m0, s[..., c.tile:2 * c.tile].max(dim=-1, keepdim=True).values)       # -inf where tile 1 holds no key of the row
        num = w.clone()
        num[..., :c.tile] *= torch.exp(m1 - m0)                        # tile 0's sum kept at its own maximum: the factor exp(m0 - m1) missing
    out = torch.einsum("rhk,hkd->rhd", num, v64.repeat_interleave(g, dim=0)) / w.sum(dim=-1, keepdim=True)
    if fault == 6 and g >= 2:
        idx = torch.arange(c.n_q)
        idx = torch.where(idx % g == 0, idx + 1, torch.where(idx % g == 1, idx - 1, idx))
        out = out[:, idx]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the assertions (the GPU test applies them to the kernels' output, the CPU test to ``reference`` with and without a fault)
# ---------------------------------------------------------------------------------------------------------------------------------
def _ulp(v, dtype):
    from test_gpu_gemv_mma import _ulp as ulp
    return ulp(v, dtype)


def check(c, got):
    """``got``: the result of the case's call (any device; [R, n_q HD], [n_q HD] or [R, n_q, HD]).  Raises AssertionError; returns the
    worst ratio of an error to its bound (0 for the needle, which has none)."""
    got = got.detach().cpu().reshape(len(c.positions), c.n_q, HD)
    assert got.dtype == c.dtype or got.dtype == torch.float64
    got = got.to(c.dtype)                                             # (the CPU test hands over fp64: one rounding to T)
    assert bool(torch.isfinite(got).all()), f"{c.label}: non-finite output"
    if c.family == "needle":
        want = c.want.to(c.dtype)
        if not torch.equal(got, want):
            bad = (got != want).any(dim=-1).nonzero()
            r, h = (int(x) for x in bad[0])
            raise AssertionError(f"{c.label}: {len(bad)} rows differ from their target's V row, first: position {c.positions[r]} head {h} "
                                 f"target {int(c.targets[r, h])}, max|d| = {float((got[r, h].double() - c.want[r, h]).abs().max()):.3g}")
        return 0.0
    g64 = got.double()
    if c.family == "counting":
        worst = 0.0
        for r, p in enumerate(c.positions):
            cd = counts(p)
            want = cd / (p + 1)
            err, bound = (g64[r] - want[None]).abs(), _ulp(want, c.dtype)[None]
            assert bool((err <= bound).all()), f"{c.label}: position {p}: {int((err > bound).sum())} elements off c_d / (p + 1) by more than one ulp"
            assert torch.equal(torch.round(g64[r] * (p + 1)), cd[None].expand(c.n_q, HD)), f"{c.label}: position {p}: a key was not counted once"
            worst = max(worst, float((err / bound).max()))
        return worst
    want = reference(c)
    err = (g64 - want).abs().amax(dim=-1)
    bound = TOL[c.dtype] * want.abs().amax(dim=-1)
    ratio = err / bound
    worst = float(ratio.max())
    if worst > 1.0:
        r, h = (int(x) for x in (ratio > 1.0).nonzero()[0])
        raise AssertionError(f"{c.label}: position {c.positions[r]} head {h}: max_d|d| = {float(err[r, h]):.3e} > {float(bound[r, h]):.3e} "
                             f"(worst ratio {worst:.3g})")
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the case lists of tests/test_gpu_caption_attention.py
# ---------------------------------------------------------------------------------------------------------------------------------
def prefill_cases(dtype, shapes=None):
    for shape in PREFILL_BASE + PREFILL_GROUPS if shapes is None else shapes:
        yield needle_prefill(shape, dtype, "table")
        yield needle_prefill(shape, dtype, "scatter")
        yield counting_prefill(shape, dtype)
        if shape in PREFILL_BASE:
            for profile in RAMP_PROFILES:
                yield ramp_prefill(shape, dtype, profile)


def decode_cases(n_q, n_kv, positions, dtype, ramp):
    """positions: [(max_len, pos)]"""
    for t, (max_len, pos) in enumerate(positions):
        yield needle_decode(n_q, n_kv, max_len, pos, t, dtype)
        yield counting_decode(n_q, n_kv, max_len, pos, dtype)
        if ramp:
            for profile in RAMP_PROFILES:
                yield ramp_decode(n_q, n_kv, max_len, pos, dtype, profile)


def combine_cases(dtype, positions=COMBINE_POSITIONS):
    return decode_cases(*COMBINE_GROUP, [(COMBINE_MAX_LEN, p) for p in positions], dtype, True)


def all_cases(dtype):
    yield from prefill_cases(dtype)
    for n_q, n_kv in DECODE_GROUPS:
        yield from decode_cases(n_q, n_kv, DECODE_POSITIONS, dtype, (n_q, n_kv) in DECODE_RAMP_GROUPS)
    yield from combine_cases(dtype)
