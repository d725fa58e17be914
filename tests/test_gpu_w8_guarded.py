"""The wrappers of rsvld_amd/w8.py on poisoned, guard-banded buffers (tests/guarded.py), mirroring the ``decode`` family of
tests/test_gpu_guarded.py: "rows past N re-read the last row, never stored", pieces past the end of K skipped per lane, the
quantiser's two passes over a row.  The result is bit-identical to the plain call.

A byte of ``q`` left unwritten shows as 0xFF.  The quantiser never writes that byte: finite weights give finite e4m3 codes, and a
non-finite one gives 0x7F.  So ``_no_poison`` is the element test of the uint8 result."""
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
CASES = [(1003, 528, F16), (1003, 528, BF16), (17, 16, F16), (17, 16, BF16), (4096, 4096, F16)]
_IDS = [f"{n}x{k}_{'f16' if d == F16 else 'bf16'}" for n, k, d in CASES]


def _no_poison(name, t):
    return (t != guarded.POISON) if t.dtype == torch.uint8 else None


def _weights(cuda, N, K, dt):
    g = torch.Generator().manual_seed(N + K)
    return (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dt), g


@pytest.mark.parametrize("N,K,dt", CASES, ids=_IDS)
def test_pack_rows_e4m3_guarded(cuda, N, K, dt):
    from rsvld_amd import w8
    w, _ = _weights(cuda, N, K, dt)
    (q, scale), _ = guarded.run_guarded(w8.pack_rows_e4m3, {"w": w}, expect="pack_rows_e4m3", finite=_no_poison)
    qh, sh = w8.pack_rows_e4m3_host(w)
    assert torch.equal(q.cpu(), qh) and torch.equal(scale.cpu(), sh)


@pytest.mark.parametrize("N,K,dt", CASES, ids=_IDS)
def test_gemv_w8_guarded(cuda, N, K, dt):
    """Plain (with a bias) and the three fused forms."""
    from rsvld_amd import w8
    w, g = _weights(cuda, N, K, dt)
    q, scale = w8.pack_rows_e4m3(w)
    x = torch.randn(K, generator=g).to(cuda, dt)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda, dt)
    nw = (torch.randn(K, generator=g) * 0.2 + 1).to(cuda, dt)
    res = torch.randn(N, generator=g).to(cuda, dt)
    gu = torch.randn(2 * K, generator=g).to(cuda, dt)

    def fn(q, scale, x, b, nw, res, gu):
        return (w8.gemv_w8(q, scale, x, b), w8.gemv_w8(q, scale, x, None, norm=(nw, 1e-5)), w8.gemv_w8(q, scale, x, None, residual=res),
                w8.gemv_w8(q, scale, gu, None, glu=True, residual=res))
    guarded.run_guarded(fn, dict(q=q, scale=scale, x=x, b=b, nw=nw, res=res, gu=gu), expect="gemv_w8")
