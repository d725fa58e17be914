"""``w8.linear_w8`` (rsvld_gemm_w8) on the GPU: exactly computable operands bit for bit against fp64, random operands inside the 16-bit
product's own bound, the row-invariance contract bit for bit, agreement with the matrix-vector kernel, and the e4m3 NaN byte.

Shapes (N, K) -- the smallest that reach the cases of a 128 x 128 x 64 tile kernel whose K comes in 16-byte pieces of 16:
  (17, 16)      one piece: one K step, three quarters of it zero-filled; one ragged column tile
  (1003, 528)   528 = 8 x 64 + 16: a last K step of ONE piece, a K that is no multiple of any plausible step; 1003 = 7 x 128 + 107
  (320, 2064)   33 K steps (the double buffer turns over many times), the last of one piece; 320 = 2.5 column tiles
  (512, 1024)   whole tiles, whole steps: no masking anywhere in N and K
M in {1, 5, 33, 257}: a single row, a few, either side of 32 (an MFMA block) and of 256 (two row tiles and one row of a third)."""
import pytest
import torch

from test_gpu_kernels import _close
from test_linear_w8_cases import EXACT_ROWS, EXACT_SHAPES, build_exact_rows

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}
_SID = lambda s: f"{s[0]}x{s[1]}"
M_RANDOM = 300

_random = {}


def random_case(cuda, dtype, N, K):
    """Random operands with M = 300 rows, their pack and the plain results -- made once per (dtype, shape) and shared, never modified."""
    key = (dtype, N, K)
    if key not in _random:
        from rsvld_amd import w8
        g = torch.Generator().manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dtype)
        x = torch.randn(M_RANDOM, K, generator=g).to(cuda, dtype)
        b = (torch.randn(N, generator=g) * 0.1).to(cuda, dtype)
        q, scale = w8.pack_rows_e4m3(w)
        _random[key] = dict(q=q, scale=scale, x=x, b=b, out=w8.linear_w8(q, scale, x), out_b=w8.linear_w8(q, scale, x, b))
    return _random[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_SID)
def test_linear_w8_exact_operands(cuda, dtype, shape):
    """``torch.equal`` against fp64, through the device quantiser (which must return the host model's bytes for these rows), with and
    without a bias, for every M; and every row equals the matrix-vector kernel's result for it (both are exact here)."""
    from rsvld_amd import w8
    N, K = shape
    q = scale = None
    for M in EXACT_ROWS:
        c = build_exact_rows(dtype, N, K, M)
        if q is None:
            q, scale = w8.pack_rows_e4m3(c["w"].to(cuda))
            assert torch.equal(q.cpu(), c["q"]) and torch.equal(scale.cpu(), c["scale"])
        x, b = c["x"].to(cuda), c["bias"].to(cuda)
        got, got_b = w8.linear_w8(q, scale, x), w8.linear_w8(q, scale, x, b)
        assert got.shape == (M, N) and got.dtype == dtype
        assert torch.equal(got.cpu(), c["want"]["plain"]), (M, "plain")
        assert torch.equal(got_b.cpu(), c["want"]["bias"]), (M, "bias")
        for m in {0, M - 1}:
            assert torch.equal(w8.gemv_w8(q, scale, x[m], b), got_b[m]), (M, m)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_SID)
def test_linear_w8_random_operands(cuda, dtype, shape):
    """Against ``x.double() @ dequant(q, scale).double().T``: after dequantisation the arithmetic is a 16-bit product with fp32 accumulation,
    so the bound is tests/test_gpu_kernels.py's ``_close`` for the dtype, as in test_gemv_w8_weight_streaming."""
    from rsvld_amd import w8
    c = random_case(cuda, dtype, *shape)
    want = (c["x"].double() @ w8.dequant(c["q"], c["scale"]).double().T).float().cpu()
    print(f"{shape} {dtype}: max|d| = {_close(c['out'], want, dtype):.3e}, with bias {_close(c['out_b'], want + c['b'].float().cpu(), dtype):.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_SID)
def test_linear_w8_row_invariance(cuda, dtype, shape):
    """``out[m]`` depends on ``x[m]`` only, bit for bit: not on M, not on the other rows (NaN included), not on the run."""
    from rsvld_amd import w8
    c = random_case(cuda, dtype, *shape)
    q, scale, x, b, full = c["q"], c["scale"], c["x"], c["b"], c["out_b"]
    assert bool(torch.isfinite(full).all())
    assert torch.equal(w8.linear_w8(q, scale, x, b), full), "two runs differ"
    for m in (1, 31, 32, 33, 255, 257):
        assert torch.equal(w8.linear_w8(q, scale, x[:m].contiguous(), b), full[:m]), m
    poisoned = torch.full_like(x, float("nan"))
    poisoned[7] = x[7]
    got = w8.linear_w8(q, scale, poisoned, b)
    assert torch.equal(got[7], full[7])
    assert bool(torch.isnan(got[:7]).all()) and bool(torch.isnan(got[8:]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_SID)
def test_linear_w8_rows_agree_with_the_gemv(cuda, dtype, shape):
    """Close, not equal: the matrix-vector kernel sums K in another order."""
    from rsvld_amd import w8
    c = random_case(cuda, dtype, *shape)
    scale_of = float(c["out_b"].float().abs().max())
    for m in (0, 7, 130, M_RANDOM - 1):
        _close(c["out_b"][m], w8.gemv_w8(c["q"], c["scale"], c["x"][m], c["b"]).float().cpu(), dtype, scale=scale_of)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
def test_linear_w8_nan_byte_marks_its_column(cuda, dtype):
    """One 0x7F (what the quantiser writes for a non-finite weight) in row n of ``q``: column n of the result is NaN in every row, and
    no other column is -- also where the activation beside the byte is zero (0 x NaN = NaN)."""
    from rsvld_amd import w8
    N, K = 1003, 528
    c = random_case(cuda, dtype, N, K)
    for n, k, byte in ((0, 0, 0x7F), (1002, 527, 0xFF), (200, 515, 0x7F)):
        q = c["q"].clone()
        q[n, k] = byte
        x = c["x"].clone()
        x[5, k] = 0
        got = w8.linear_w8(q, c["scale"], x, c["b"])
        assert bool(torch.isnan(got[:, n]).all()), (n, k)
        keep = torch.ones(N, dtype=torch.bool, device=cuda)
        keep[n] = False
        assert bool(torch.isfinite(got[:, keep]).all()), (n, k)
        rows = torch.ones(M_RANDOM, dtype=torch.bool, device=cuda)
        rows[5] = False
        assert torch.equal(got[rows][:, keep], c["out_b"][rows][:, keep])
