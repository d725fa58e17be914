"""Causal grouped-query flash attention over one sequence's static key / value cache (rsvld_llama_prefill_attention,
csrc/prefill_attention.hip): the attention of the caption pass's PREFILL, the opt-in ``llava_next.FastDecoder(prefill="flash")`` /
``--caption_prefill flash``.  It stands where ``FastDecoder.forward`` otherwise multiplies the prompt's queries against the WHOLE cache of
``max_len`` positions under an additive mask and materialises the fp32 scores: here a query row reads keys ``0 .. its own position`` in a
fixed order, no score or mask tensor exists, and the stale tail of the cache is never read.

Contract (include/rsvld_hip.h): output row ``t`` is a function of ``q[t]`` and of keys / values ``0 .. pos0 + t`` of its kv head only -- bit
for bit the same whatever ``T``, the other rows of the call, ``max_len`` and the cache contents above the call's last position (NaN
included) are; tests/test_gpu_prefill_attention.py compares with ``torch.equal``.

Like every wrapper of ``ops``: operands are checked before anything is allocated or launched, a CPU tensor raises (there is no CPU
path and no fallback to torch), the launch goes through ``ops._launch``."""
from . import _lib as L
from . import ops


def llama_prefill_attention(q, kcache, vcache, n_q, n_kv, scale, pos0=0):
    """``q [T, n_q * 128]`` (or ``[T, n_q, 128]``; rotary embedding applied; unit inner stride, any 16-byte token stride: a column slice of
    the fused q | k tensor is taken as it is) at positions ``pos0 .. pos0 + T - 1``; ``kcache`` / ``vcache [n_kv, max_len, 128]`` contiguous,
    read only, already holding positions ``0 .. pos0 + T - 1``; ``pos0`` a host int.  -> ``out [T, n_q * 128]``, row ``t`` =
    ``softmax(q[t] K^T scale) V`` over keys ``0 .. pos0 + t`` of head ``h``'s kv head ``h // (n_q // n_kv)``.  head_dim 128, at most 8 query
    heads per kv head, fp16 / bf16: anything else raises."""
    return ops._prefill_attention("llama_prefill_attention", q, kcache, vcache, n_q, n_kv, scale, pos0)


def plan(T, n_q, n_kv, head_dim=128):
    """The launch of such a call (rsvld_plan_llama_prefill_attention, host only): ``_lib.PrefillAttentionPlan`` -- a function of
    ``(T, n_q, n_kv)`` alone."""
    pl = L.PrefillAttentionPlan()
    L.check(L.load().rsvld_plan_llama_prefill_attention(int(T), int(n_q), int(n_kv), int(head_dim), pl), "rsvld_plan_llama_prefill_attention")
    return pl
