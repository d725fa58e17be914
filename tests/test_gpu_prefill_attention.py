"""rsvld_llama_prefill_attention (csrc/prefill_attention.hip) through rsvld_amd.prefill_attention: the kernel against a CPU fp32 causal
softmax attention on inputs pre-rounded to the storage type, under the bound of tests/test_gpu_kernels.py::_close (4e-3 fp16, 3e-2 bf16,
times max|want|, plus 1e-6), and its contract with ``torch.equal``: a row's result does not depend on T, on the other rows of the call,
on max_len or on what the cache holds above the call's last position (NaN included), and two runs are bit-identical."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
HD = 128
# (T, pos0, n_q, n_kv, max_len)
CASES = [(1, 0, 8, 2, 64),
         (33, 0, 8, 2, 64),        # a ragged row block, the diagonal inside one key tile
         (64, 0, 4, 4, 64),        # g = 1, T = max_len: the last slot is used
         (129, 0, 8, 1, 256),      # g = 8, three key tiles
         (300, 0, 8, 2, 384),
         (60, 100, 8, 2, 192)]     # pos0 > 0, the diagonal straddles a tile boundary
_IDS = ["t%d_p%d_q%d_kv%d_m%d" % c for c in CASES]
TOL = {F16: 4e-3, BF16: 3e-2}


@functools.lru_cache(maxsize=None)
def _inputs(T, pos0, n_q, n_kv, max_len, dtype):
    """q [T, n_q, HD] and caches [n_kv, max_len, HD] on the host, rounded to ``dtype``: the cache is random in EVERY slot (the slots above
    pos0 + T - 1 are stale contents the kernel must not use).  Shared by the tests, never modified (callers clone)."""
    g = torch.Generator().manual_seed(1000 * T + 10 * pos0 + n_q + n_kv)
    q = torch.randn(T, n_q, HD, generator=g).to(dtype)
    k = torch.randn(n_kv, max_len, HD, generator=g).to(dtype)
    v = torch.randn(n_kv, max_len, HD, generator=g).to(dtype)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _reference(T, pos0, n_q, n_kv, max_len, dtype):
    """CPU fp32 causal softmax attention of the rounded inputs -> [T, n_q * HD] fp32."""
    q, k, v = (t.float() for t in _inputs(T, pos0, n_q, n_kv, max_len, dtype))
    g = n_q // n_kv
    n = pos0 + T
    kk, vv = k[:, :n].repeat_interleave(g, dim=0), v[:, :n].repeat_interleave(g, dim=0)      # [n_q, n, HD]
    s = torch.einsum("thd,hkd->thk", q, kk) * HD ** -0.5
    keys, rows = torch.arange(n)[None, None, :], (pos0 + torch.arange(T))[:, None, None]
    s = s.masked_fill(keys > rows, float("-inf"))
    return torch.einsum("thk,hkd->thd", torch.softmax(s, dim=-1), vv).reshape(T, n_q * HD)


def _run(cuda, q, k, v, n_q, n_kv, pos0=0):
    from rsvld_amd import prefill_attention as PA
    return PA.llama_prefill_attention(q.to(cuda), k.to(cuda), v.to(cuda), n_q, n_kv, HD ** -0.5, pos0=pos0)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_kernel_against_cpu_fp32_reference(cuda, case, dtype):
    T, pos0, n_q, n_kv, max_len = case
    q, k, v = _inputs(*case, dtype)
    got = _run(cuda, q, k, v, n_q, n_kv, pos0)
    assert got.shape == (T, n_q * HD) and got.dtype == dtype and got.is_contiguous()
    want = _reference(*case, dtype)
    err = float((got.float().cpu() - want).abs().max())
    bound = TOL[dtype] * float(want.abs().max()) + 1e-6
    print(f"prefill attention {case} {dtype}: max|d| = {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_strided_q_view_of_a_fused_qk_tensor(cuda, dtype):
    """q as FastDecoder.forward hands it over: the first n_q heads of a [T, n_q + n_kv, HD] tensor."""
    case = (60, 100, 8, 2, 192)
    q, k, v = _inputs(*case, dtype)
    qk = torch.cat([q, torch.full((60, 2, HD), float("nan"), dtype=dtype)], dim=1).to(cuda)
    from rsvld_amd import prefill_attention as PA
    got = PA.llama_prefill_attention(qk[:, :8], k.to(cuda), v.to(cuda), 8, 2, HD ** -0.5, pos0=100)
    assert torch.equal(got, _run(cuda, q, k, v, 8, 2, 100))


@pytest.fixture(scope="module")
def base300(cuda):
    """The (300, 0, 8, 2, 384) case in fp16 and its output, computed once."""
    case = (300, 0, 8, 2, 384)
    q, k, v = _inputs(*case, F16)
    return q, k, v, _run(cuda, q, k, v, 8, 2)


def test_output_does_not_depend_on_max_len(cuda, base300):
    q, k, v, out = base300
    g = torch.Generator().manual_seed(5)
    k2 = torch.cat([k, torch.randn(2, 256, HD, generator=g).half()], dim=1)
    v2 = torch.cat([v, torch.randn(2, 256, HD, generator=g).half()], dim=1)
    assert k2.shape[1] == 640
    assert torch.equal(_run(cuda, q, k2, v2, 8, 2), out)


def test_output_does_not_depend_on_the_cache_above_the_last_position(cuda, base300):
    q, k, v, out = base300
    k2, v2 = k.clone(), v.clone()
    k2[:, 300:] = float("nan")
    v2[:, 300:] = float("nan")
    got = _run(cuda, q, k2, v2, 8, 2)
    assert torch.isfinite(got).all()
    assert torch.equal(got, out)


def test_one_call_equals_two_calls_at_consecutive_positions(cuda, base300):
    q, k, v, out = base300
    a = _run(cuda, q[:137], k, v, 8, 2, pos0=0)
    b = _run(cuda, q[137:], k, v, 8, 2, pos0=137)
    assert b.shape[0] == 163
    assert torch.equal(torch.cat([a, b]), out)


def test_rows_do_not_depend_on_T(cuda, base300):
    """Rows 0..99 of the T = 300 call = a T = 100 call -- over the same cache, and over one whose slots above 99 hold NaN."""
    q, k, v, out = base300
    assert torch.equal(_run(cuda, q[:100], k, v, 8, 2), out[:100])
    k2, v2 = k.clone(), v.clone()
    k2[:, 100:] = float("nan")
    v2[:, 100:] = float("nan")
    assert torch.equal(_run(cuda, q[:100], k2, v2, 8, 2), out[:100])


def test_two_runs_are_bit_identical(cuda, base300):
    q, k, v, out = base300
    assert torch.equal(_run(cuda, q, k, v, 8, 2), out)


def test_refusals(cuda):
    from rsvld_amd import _lib
    from rsvld_amd import prefill_attention as PA
    z = lambda *s, dt=F16: torch.zeros(*s, device=cuda, dtype=dt)
    with pytest.raises((_lib.RsvldError, ValueError)):                       # head_dim 64
        PA.llama_prefill_attention(z(4, 8 * 64), z(2, 64, 64), z(2, 64, 64), 8, 2, 0.1)
    with pytest.raises((_lib.RsvldError, ValueError)):                       # 16 query heads per kv head
        PA.llama_prefill_attention(z(4, 16 * HD), z(1, 64, HD), z(1, 64, HD), 16, 1, 0.1)
    with pytest.raises((_lib.RsvldError, ValueError)):                       # pos0 + T > max_len
        PA.llama_prefill_attention(z(4, 8 * HD), z(2, 64, HD), z(2, 64, HD), 8, 2, 0.1, pos0=61)
    with pytest.raises((_lib.RsvldError, ValueError)):                       # fp32
        PA.llama_prefill_attention(z(4, 8 * HD, dt=torch.float32), z(2, 64, HD, dt=torch.float32), z(2, 64, HD, dt=torch.float32), 8, 2, 0.1)
    with pytest.raises((_lib.RsvldError, ValueError)):                       # a negative first position
        PA.llama_prefill_attention(z(4, 8 * HD), z(2, 64, HD), z(2, 64, HD), 8, 2, 0.1, pos0=-1)
