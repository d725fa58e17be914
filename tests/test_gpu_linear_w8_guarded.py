"""``w8.linear_w8`` on poisoned, guard-banded buffers (tests/guarded.py), as tests/test_gpu_w8_guarded.py does for the matrix-vector
kernel: the promises of csrc/gemm_w8.hip about memory outside its operands -- rows past M, columns past N and K pieces past K are zeros
in LDS, "never loaded", and their results are "not stored".  Ragged M, N and K against the 128 x 128 x 64 tile; nothing outside ``out``
is written, no operand is modified, no poison reaches a result, and the result is bit-identical to the plain call."""
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# (M, N, K): one row / one piece; every edge ragged, K ending in a single piece; M and N one past a tile; whole tiles
CASES = [(1, 17, 16, F16), (33, 1003, 528, BF16), (129, 129, 80, F16), (5, 320, 2064, BF16), (257, 130, 1040, F16), (128, 256, 128, BF16)]
_IDS = [f"{m}x{n}x{k}_{'f16' if d == F16 else 'bf16'}" for m, n, k, d in CASES]


@pytest.mark.parametrize("M,N,K,dt", CASES, ids=_IDS)
def test_linear_w8_guarded(cuda, M, N, K, dt):
    from rsvld_amd import w8
    g = torch.Generator().manual_seed(M + N + K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dt)
    q, scale = w8.pack_rows_e4m3(w)
    x = torch.randn(M, K, generator=g).to(cuda, dt)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda, dt)

    def fn(q, scale, x, b):
        return w8.linear_w8(q, scale, x, b), w8.linear_w8(q, scale, x)
    guarded.run_guarded(fn, dict(q=q, scale=scale, x=x, b=b), expect="linear_w8")
