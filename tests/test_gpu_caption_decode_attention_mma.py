"""The decode-step attention on MFMAs (dam_kernel of csrc/decode_attention.hip through ops.llama_decode_attention(kernel="mfma") and
decode_rows.llama_decode_attention_rows(kernel="mfma")), fp16 and bf16, against its contract in include/rsvld_hip.h.

  1  the exact families of tests/caption_attention_cases.py at every group size 1 .. 8 and at the positions
     tests/test_caption_attention_mode_cases.py proves fair and sharp: both sides of every 32-key wave block, of the 64-key tile and
     of the first two range boundaries (the range taken from the plan), the last slot, caches shorter than a range and than a tile.
     needle: ``torch.equal``; counting: one spacing of T, every key counted once; ramp: 4e-3 / 3e-2 per row against an fp64 softmax
  2  66 ranges, da_combine_kernel's second round: single calls, and B = 3 through the rows entry bit-equal to them
  3  invariance, all ``torch.equal``: row b at B = 1 .. 8, beside NaN neighbours, at another max_len, under NaN above pos, twice
  4  the caches end bit for bit as the VALU operator leaves them; both outputs within the suite's bound of an fp64 softmax
  5  poisoned, guard-banded buffers (tests/guarded.py): workspace with the rotated q, caches, out
  6  what the contract refuses raises before any launch

Measured maxima of error / bound (MI355X, every case below; fp16 / bf16), the needle being equal everywhere:
    exact families    counting 0.49 / 0.25   ramp 0.13 / 0.16
    66 ranges         counting 0.26 / 0.22   ramp 0.10 / 0.13
    random operands   this operator 0.13 / 0.16, the VALU operator 0.23 / 0.26 of the per-row bound against the fp64 softmax
No case failed when these tests were first run."""
import pytest
import torch

import caption_attention_cases as CA
import guarded
from test_caption_attention_mode_cases import combine_shape, plan, positions
from test_gpu_caption_attention import _check_cache, _walk

pytestmark = pytest.mark.gpu

HD = CA.HD
_DT = pytest.mark.parametrize("dtype", CA.DTYPES, ids=CA.DTN.get)


def _decode(cuda, c, kernel="mfma"):
    from rsvld_amd import ops
    kc, vc = c.kc.to(cuda), c.vc.to(cuda)
    k0, v0 = kc.clone(), vc.clone()
    got = ops.llama_decode_attention(c.qkv.to(cuda), c.cos.to(cuda), c.sin.to(cuda), torch.tensor([c.pos], device=cuda), kc, vc,
                                     c.n_q, c.n_kv, CA.SCALE, kernel=kernel)
    assert got.shape == (c.n_q * HD,) and got.dtype == c.dtype
    _check_cache(c, kc, vc, k0, v0)
    return got


# ---- 1
@_DT
@pytest.mark.parametrize("group", CA.DECODE_GROUPS, ids=lambda g: "q%d_kv%d" % g)
def test_exact_families_at_every_wave_tile_and_range_boundary(cuda, group, dtype):
    R = int(plan(*group, 384, dtype).range_keys)
    cases = CA.decode_cases(*group, positions(R), dtype, group in CA.DECODE_RAMP_GROUPS)
    print(_walk(cases, lambda c: _decode(cuda, c)))


# ---- 2
@_DT
def test_combine_second_round(cuda, dtype):
    n_q, n_kv = CA.COMBINE_GROUP
    max_len, pos = combine_shape(int(plan(n_q, n_kv, 384, dtype).range_keys))
    assert plan(n_q, n_kv, max_len, dtype).ranges == 66
    print(_walk(CA.decode_cases(n_q, n_kv, [(max_len, p) for p in pos], dtype, True), lambda c: _decode(cuda, c)))


@_DT
def test_combine_second_round_rows_equal_single_calls(cuda, dtype):
    from rsvld_amd import decode_rows as DR
    n_q, n_kv = CA.COMBINE_GROUP
    max_len, pos = combine_shape(int(plan(n_q, n_kv, 384, dtype).range_keys))
    rows = [pos[0], pos[2], pos[3]]
    by_family = {}
    for c in CA.decode_cases(n_q, n_kv, [(max_len, p) for p in rows], dtype, True):
        by_family.setdefault(c.label.split()[-1], []).append(c)
    assert sorted(by_family) == ["counting", "needle", "ramp/saw", "ramp/up"]
    for name, cs in by_family.items():
        want = torch.stack([_decode(cuda, c) for c in cs])
        kb, vb = torch.stack([c.kc for c in cs]).to(cuda), torch.stack([c.vc for c in cs]).to(cuda)
        k0, v0 = kb.clone(), vb.clone()
        got = DR.llama_decode_attention_rows(torch.stack([c.qkv for c in cs]).to(cuda), torch.stack([c.cos for c in cs]).to(cuda),
                                             torch.stack([c.sin for c in cs]).to(cuda), torch.tensor(rows, device=cuda), kb, vb,
                                             n_q, n_kv, CA.SCALE, kernel="mfma")
        assert torch.equal(got, want), name
        for b, c in enumerate(cs):
            _check_cache(c, kb[b], vb[b], k0[b], v0[b])
            CA.check(c, got[b])


# ---- 3, 4: random operands, eight sequences at different positions
N_Q, N_KV, MAX_LEN = 8, 2, 384
POS8 = [0, 31, 127, 128, 200, 255, 256, 383]


def _random(dtype, max_len=MAX_LEN, seed=7):
    g = torch.Generator().manual_seed(seed)
    B = len(POS8)
    qkv = torch.randn(B, (N_Q + 2 * N_KV) * HD, generator=g).to(dtype)
    kc, vc = torch.randn(B, N_KV, MAX_LEN, HD, generator=g).to(dtype), torch.randn(B, N_KV, MAX_LEN, HD, generator=g).to(dtype)
    ang = torch.rand(B, HD // 2, generator=g) * 6
    cos, sin = torch.cat([ang.cos(), ang.cos()], dim=1).to(dtype), torch.cat([ang.sin(), ang.sin()], dim=1).to(dtype)
    if max_len != MAX_LEN:                                          # the same sequences in a longer cache
        k2, v2 = torch.zeros(B, N_KV, max_len, HD, dtype=dtype), torch.zeros(B, N_KV, max_len, HD, dtype=dtype)
        k2[:, :, :MAX_LEN], v2[:, :, :MAX_LEN] = kc, vc
        kc, vc = k2, v2
    return qkv, cos, sin, torch.tensor(POS8), kc, vc


def _rows(cuda, ops_, rows=slice(None), kernel="mfma"):
    """The rows entry on sequences ``rows`` of the operands -> (out, kcache, vcache) after the call."""
    from rsvld_amd import decode_rows as DR
    qkv, cos, sin, pos, kc, vc = (t[rows].to(cuda).contiguous() for t in ops_)
    out = DR.llama_decode_attention_rows(qkv, cos, sin, pos, kc, vc, N_Q, N_KV, HD ** -0.5, kernel=kernel)
    return out, kc, vc


def _written(kc, vc, pos):
    b = torch.arange(len(pos))
    return kc[b, :, pos.to(kc.device)], vc[b, :, pos.to(kc.device)]


@_DT
def test_row_b_is_the_same_at_every_row_count_and_twice(cuda, dtype):
    ops_ = _random(dtype)
    out8, k8, v8 = _rows(cuda, ops_)
    assert bool(torch.isfinite(out8).all())
    again = _rows(cuda, ops_)
    assert all(torch.equal(a, b) for a, b in zip((out8, k8, v8), again))
    for B in range(1, 8):
        out, kc, vc = _rows(cuda, ops_, slice(0, B))
        assert torch.equal(out, out8[:B]) and torch.equal(kc, k8[:B]) and torch.equal(vc, v8[:B]), B
    for b in (3, 7):                                                 # and alone, from another place of the batch
        out, kc, vc = _rows(cuda, ops_, slice(b, b + 1))
        assert torch.equal(out[0], out8[b]) and torch.equal(kc[0], k8[b]) and torch.equal(vc[0], v8[b]), b


@_DT
def test_row_b_beside_nan_sequences(cuda, dtype):
    ops_ = _random(dtype)
    out8, k8, v8 = _rows(cuda, ops_)
    for b in (0, 4, 7):
        qkv, cos, sin, pos, kc, vc = (t.clone() for t in ops_)
        others = torch.arange(len(POS8)) != b
        qkv[others], kc[others], vc[others] = float("nan"), float("nan"), float("nan")
        out, kc, vc = _rows(cuda, (qkv, cos, sin, pos, kc, vc))
        assert torch.equal(out[b], out8[b]) and torch.equal(kc[b], k8[b]) and torch.equal(vc[b], v8[b]), b


@_DT
def test_max_len_and_what_lies_above_pos_do_not_matter(cuda, dtype):
    ops_ = _random(dtype)
    out8, k8, v8 = _rows(cuda, ops_)
    pos = ops_[3]
    out, kc, vc = _rows(cuda, _random(dtype, max_len=640))
    assert torch.equal(out, out8) and torch.equal(kc[:, :, :MAX_LEN], k8) and torch.equal(vc[:, :, :MAX_LEN], v8)
    qkv, cos, sin, pos, kc, vc = (t.clone() for t in ops_)
    for b, p in enumerate(POS8):
        kc[b, :, p + 1:], vc[b, :, p + 1:] = float("nan"), float("nan")
    out, kc, vc = _rows(cuda, (qkv, cos, sin, pos, kc, vc))
    assert torch.equal(out, out8)
    assert all(torch.equal(a, b) for a, b in zip(_written(kc, vc, pos), _written(k8, v8, pos)))


def _rope_T(x, cos, sin, dtype):
    """da_rope on the CPU: T(x cos) + T(rot(x) sin) -> T, every product and the sum in fp32."""
    xf = x.float()
    rot = torch.cat((-xf[..., HD // 2:], xf[..., :HD // 2]), dim=-1)
    a, b = (xf * cos.float()).to(dtype).float(), (rot * sin.float()).to(dtype).float()
    return (a + b).to(dtype)


@_DT
def test_caches_equal_valu_and_both_outputs_are_within_the_bound(cuda, dtype):
    ops_ = _random(dtype)
    qkv, cos, sin, pos, kc0, vc0 = ops_
    out_m, k_m, v_m = _rows(cuda, ops_)
    out_v, k_v, v_v = _rows(cuda, ops_, kernel="valu")
    assert torch.equal(k_m, k_v) and torch.equal(v_m, v_v)
    B, g = len(POS8), N_Q // N_KV
    heads = qkv.view(B, N_Q + 2 * N_KV, HD)
    rot = _rope_T(heads[:, :N_Q + N_KV], cos[:, None], sin[:, None], dtype)
    k_new, v_new = _written(k_m.cpu(), v_m.cpu(), pos)
    assert torch.equal(k_new, rot[:, N_Q:]) and torch.equal(v_new, heads[:, N_Q + N_KV:])
    for b, p in enumerate(POS8):
        k, v = k_m[b, :, :p + 1].cpu().double().repeat_interleave(g, dim=0), v_m[b, :, :p + 1].cpu().double().repeat_interleave(g, dim=0)
        w = torch.softmax(torch.einsum("hd,hkd->hk", rot[b, :N_Q].double(), k) * HD ** -0.5, dim=-1)
        want = torch.einsum("hk,hkd->hd", w, v)
        bound = CA.TOL[dtype] * want.abs().amax(dim=-1)
        for name, out in (("mfma", out_m), ("valu", out_v)):
            err = (out[b].cpu().double().view(N_Q, HD) - want).abs().amax(dim=-1)
            print(f"{name} {CA.DTN[dtype]} pos {p}: worst error / bound = {float((err / bound).max()):.3g}")
            assert bool((err <= bound).all()), (name, p, float((err / bound).max()))


# ---- 5
@pytest.mark.parametrize("dt", CA.DTYPES, ids=CA.DTN.get)
@pytest.mark.parametrize("nq,nkv,max_len,pos", [(8, 2, 777, (0, 255, 256, 300, 127, 128, 5, 776)), (8, 1, 384, (0, 128, 383)),
                                                (2, 1, 8325, (100, 8192, 8324))], ids=["b8_len777", "q8_kv1_len384", "q2_kv1_len8325"])
def test_guarded(cuda, nq, nkv, max_len, pos, dt):
    """Every slot above a sequence's position holds 0xFF bytes, the last sequence's write lands flush against the end of both caches;
    the workspace (rotated q, then the partials) and the output are allocated under the proxy: poison until written."""
    from rsvld_amd import decode_rows as DR
    B = len(pos)
    g = torch.Generator().manual_seed(max_len)
    qkv = torch.randn(B, (nq + 2 * nkv) * HD, generator=g).to(cuda, dt)
    kc, vc = torch.randn(B, nkv, max_len, HD, generator=g).to(cuda, dt), torch.randn(B, nkv, max_len, HD, generator=g).to(cuda, dt)
    ang = torch.rand(B, HD // 2, generator=g) * 6
    cos, sin = torch.cat([ang.cos(), ang.cos()], dim=1).to(cuda, dt), torch.cat([ang.sin(), ang.sin()], dim=1).to(cuda, dt)
    mask = torch.zeros(B, nkv, max_len, HD, dtype=torch.bool)
    for b, p in enumerate(pos):
        kc.view(torch.int16)[b, :, p + 1:] = -1
        vc.view(torch.int16)[b, :, p + 1:] = -1
        mask[b, :, p] = True
    fn = lambda qkv, cos, sin, p, kc, vc: DR.llama_decode_attention_rows(qkv, cos, sin, p, kc, vc, nq, nkv, HD ** -0.5, kernel="mfma")
    guarded.run_guarded(fn, dict(qkv=qkv, cos=cos, sin=sin, p=torch.tensor(pos, device=cuda), kc=guarded.Op(kc, inplace=mask),
                                 vc=guarded.Op(vc, inplace=mask)), expect="llama_decode_attention_mma_rows")


# ---- 6
def test_contracts_raise_before_any_launch(cuda):
    from rsvld_amd import _lib, decode_rows as DR, ops
    dt = torch.float16

    def call(B=1, n_q=8, n_kv=2, hd=HD, max_len=64, dev=cuda, ws=None):
        z = lambda *s: torch.zeros(*s, device=dev, dtype=dt)
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            try:
                DR.llama_decode_attention_rows(z(B, (n_q + 2 * n_kv) * hd), z(B, hd), z(B, hd), torch.zeros(B, dtype=torch.int64, device=dev),
                                               z(B, n_kv, max_len, hd), z(B, n_kv, max_len, hd), n_q, n_kv, 1.0, ws=ws, kernel="mfma")
            finally:
                launched = [r[0] for r in prof.records]
        return launched

    assert call() == ["llama_decode_attention_mma_rows"]
    with pytest.raises(_lib.RsvldOperandError):
        call(B=9)
    with pytest.raises(_lib.RsvldError, match="UNSUPPORTED"):
        call(hd=64)
    with pytest.raises(_lib.RsvldError, match="UNSUPPORTED"):
        call(n_q=9, n_kv=1)
    with pytest.raises(_lib.RsvldError):
        call(dev="cpu")
    with pytest.raises(_lib.RsvldOperandError, match="ws"):
        call(ws=torch.zeros(16, device=cuda, dtype=torch.float32))
