"""The wrappers of rsvld_amd/decode_rows.py on poisoned, guard-banded buffers (tests/guarded.py, used as it is), as
tests/test_gpu_w8_guarded.py runs their single-row siblings: weight rows past N re-read the last row and are never stored, pieces
past the end of K are skipped per lane, the staged rows of several sequences lie side by side in LDS and their results side by
side in ``y`` -- flush against the rear guard after the last sequence -- and a sequence's cache slice is written at its own
position only.  The result is bit-identical to the plain call."""
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
CASES = [(N, K, B, dt) for (N, K) in ((1003, 528), (17, 16), (24, 14336)) for B in (3, 8) for dt in (F16, BF16)]
_IDS = [f"{n}x{k}_b{b}_{'f16' if d == F16 else 'bf16'}" for n, k, b, d in CASES]


def _operands(cuda, N, K, B, dt):
    g = torch.Generator().manual_seed(N + K + B)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dt)
    x = torch.randn(B, K, generator=g).to(cuda, dt)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda, dt)
    nw = (torch.randn(K, generator=g) * 0.2 + 1).to(cuda, dt)
    res = torch.randn(B, N, generator=g).to(cuda, dt)
    gu = torch.randn(B, 2 * K, generator=g).to(cuda, dt)
    return w, dict(x=x, b=b, nw=nw, res=res, gu=gu)


@pytest.mark.parametrize("N,K,B,dt", CASES, ids=_IDS)
def test_gemv_rows_guarded(cuda, N, K, B, dt):
    """Plain (with a bias) and the three fused forms."""
    from rsvld_amd import decode_rows as DR
    w, rest = _operands(cuda, N, K, B, dt)

    def fn(w, x, b, nw, res, gu):
        return (DR.gemv_rows(w, x, b), DR.gemv_rows(w, x, None, norm=(nw, 1e-5)), DR.gemv_rows(w, x, None, residual=res),
                DR.gemv_rows(w, gu, None, glu=True, residual=res))
    guarded.run_guarded(fn, dict(w=w, **rest), expect="gemv_rows")


@pytest.mark.parametrize("N,K,B,dt", CASES, ids=_IDS)
def test_gemv_w8_rows_guarded(cuda, N, K, B, dt):
    from rsvld_amd import decode_rows as DR, w8
    w, rest = _operands(cuda, N, K, B, dt)
    q, scale = w8.pack_rows_e4m3(w)

    def fn(q, scale, x, b, nw, res, gu):
        return (DR.gemv_w8_rows(q, scale, x, b), DR.gemv_w8_rows(q, scale, x, None, norm=(nw, 1e-5)),
                DR.gemv_w8_rows(q, scale, x, None, residual=res), DR.gemv_w8_rows(q, scale, gu, None, glu=True, residual=res))
    guarded.run_guarded(fn, dict(q=q, scale=scale, **rest), expect="gemv_w8_rows")


def _attention_rows_guarded(cuda, nq, nkv, max_len, positions, dt, seed):
    """Every slot beyond a sequence's position holds 0xFF bytes; the scratch is allocated under the proxy (poison)."""
    from rsvld_amd import decode_rows as DR
    B, hd = len(positions), 128
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, (nq + 2 * nkv) * hd, generator=g).to(cuda, dt)
    kc, vc = torch.randn(B, nkv, max_len, hd, generator=g).to(cuda, dt), torch.randn(B, nkv, max_len, hd, generator=g).to(cuda, dt)
    ang = torch.rand(B, hd // 2, generator=g) * 6
    cos, sin = torch.cat([ang.cos(), ang.cos()], dim=1).to(cuda, dt), torch.cat([ang.sin(), ang.sin()], dim=1).to(cuda, dt)
    mask = torch.zeros(B, nkv, max_len, hd, dtype=torch.bool)
    for b, p in enumerate(positions):
        kc.view(torch.int16)[b, :, p + 1:] = -1
        vc.view(torch.int16)[b, :, p + 1:] = -1
        mask[b, :, p] = True
    fn = lambda qkv, cos, sin, p, kc, vc: DR.llama_decode_attention_rows(qkv, cos, sin, p, kc, vc, nq, nkv, hd ** -0.5)
    guarded.run_guarded(fn, dict(qkv=qkv, cos=cos, sin=sin, p=torch.tensor(positions, device=cuda), kc=guarded.Op(kc, inplace=mask),
                                 vc=guarded.Op(vc, inplace=mask)), expect="llama_decode_attention_rows")


@pytest.mark.parametrize("B,dt", [(3, F16), (3, BF16), (8, F16), (8, BF16)], ids=["b3_f16", "b3_bf16", "b8_f16", "b8_bf16"])
def test_llama_decode_attention_rows_guarded(cuda, B, dt):
    """Positions 0, the last slot (the write of the LAST sequence lands flush against the end of both caches) and chunk boundaries
    between."""
    _attention_rows_guarded(cuda, 8, 2, 777, [0, 255, 256, 300, 127, 128, 5, 776][:B - 1] + [776], dt, seed=B)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("nq,nkv,max_len,positions", [(8, 1, 384, (0, 128, 383)), (2, 1, 8325, (100, 8192, 8324))],
                         ids=["q8_kv1_len384", "q2_kv1_len8325"])
def test_llama_decode_attention_rows_guarded_group_of_8_and_66_chunks(cuda, nq, nkv, max_len, positions, dt):
    """B = 3.  Eight query heads on ONE kv head: the per-head loops of da_kernel take their second pass and a chunk's partials are 8 rows
    of the workspace.  max_len = 8325 is 66 key chunks: da_combine_kernel's second round, with the round empty (100), one key in it
    (8192) and the last slot flush against the end of both caches (8324)."""
    _attention_rows_guarded(cuda, nq, nkv, max_len, list(positions), dt, seed=max_len)
