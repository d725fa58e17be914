"""rsvld_amd.prefill_attention.llama_prefill_attention on poisoned, guard-banded buffers (tests/guarded.py, used as it is), the way
tests/test_gpu_decode_rows_guarded.py runs the decode-step operators: q is the strided column slice of a fused q | k tensor, placed with
0xFF (NaN) bytes in the gaps between its token rows; both caches are read-only operands (``check_operands``: not one byte modified) whose
slots above the call's last position hold 0xFF bytes, the last kv head's slice ending flush against the rear guard; the output is
allocated under the proxy (poison) and must come back finite in every element -- every element written, no poison consumed -- and
bit-identical to the plain call."""
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
HD = 128
# (T, pos0, n_q, n_kv, max_len) of tests/test_gpu_prefill_attention.py, and g = 3 of tests/test_gpu_caption_attention.py: 128 rows per
# workgroup and 32 per wave are no multiple of 3, one token's heads straddle two waves
CASES = [(33, 0, 8, 2, 64), (60, 100, 8, 2, 192), (45, 0, 3, 1, 64)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["t33_p0", "t60_p100", "t45_p0_g3"])
def test_llama_prefill_attention_guarded(cuda, case, dtype):
    from rsvld_amd import prefill_attention as PA
    T, pos0, n_q, n_kv, max_len = case
    g = torch.Generator().manual_seed(T + pos0)
    qk = torch.randn(T, n_q + n_kv, HD, generator=g).to(cuda, dtype)
    q = qk[:, :n_q]                                                    # token stride (n_q + n_kv) * HD, the k columns are the gaps
    kc, vc = torch.randn(n_kv, max_len, HD, generator=g).to(cuda, dtype), torch.randn(n_kv, max_len, HD, generator=g).to(cuda, dtype)
    kc.view(torch.int16)[:, pos0 + T:] = -1                            # stale slots: 0xFF bytes
    vc.view(torch.int16)[:, pos0 + T:] = -1
    fn = lambda q, kc, vc: PA.llama_prefill_attention(q, kc, vc, n_q, n_kv, HD ** -0.5, pos0=pos0)
    got, rec = guarded.run_guarded(fn, dict(q=guarded.Op(q, view=True), kc=kc, vc=vc), expect="llama_prefill_attention")
    assert got.shape == (T, n_q * HD)
    # the operands are read-only: verdict 2 once more, by name (run_guarded has already given all four verdicts)
    rec.arena.check_operands()
    assert all(r.may_change is None for r in rec.arena.regions if r.kind == "operand")
