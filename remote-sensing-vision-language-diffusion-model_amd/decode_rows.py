"""The decode-step operators for SEVERAL independent sequences at once (rsvld_gemv_rows_fused, rsvld_gemv_w8_rows_fused,
rsvld_llama_decode_attention_rows): the batched token loop of the caption pass (``llava_next.FastDecoder(batch=B)``,
``infer_dir --caption_batch``), which streams the decoder's weights once per token for up to ``MAX_ROWS`` captions.

Each operator has ONE implementation (``ops._gemv_rows``, ``ops._decode_attention_rows``) and one host path in the library; this module is
its ``[B, .]`` face, and ``ops.gemv_fused``, ``w8.gemv_w8`` and ``ops.llama_decode_attention`` are its ``B = 1`` case.  Contract: row ``b`` of every
result is bit for bit what the single-row function returns for row ``b`` alone, whatever ``B`` is and whatever the other rows hold
(tests/test_gpu_decode_rows.py compares with ``torch.equal``).  Every operand is checked before anything is allocated or launched, a CPU
tensor raises (there is no CPU path), launches go through ``ops._launch``."""
from . import _lib as L   # noqa: F401
from . import ops
from .ops import MAX_ROWS   # noqa: F401
from .w8 import gemv_w8_rows   # noqa: F401


def gemv_rows(w, x, bias=None, *, norm=None, residual=None, glu=False, kernel="valu"):
    """``ops.gemv_fused`` for ``B`` activation rows (rsvld_gemv_rows_fused): ``w [N, K]`` 16-bit, ``x [B, K]`` (``[B, 2 K]`` = gate | up
    with ``glu``), ``residual [B, N]``; ``bias [N]`` and ``norm=(weight [K], eps)`` are shared by the rows.  -> ``[B, N]``.
    ``kernel="mfma"`` (opt-in): the product on MFMAs (rsvld_gemv_mma_rows_fused, csrc/gemv_mma.hip), at every ``B`` including 1: the same
    staged rows and epilogue roundings, the fp32 sum in another order -- row ``b`` bit-identical among ITS row counts, not to "valu"."""
    return ops._gemv_rows("gemv_rows", "gemv_rows" if kernel == "valu" else "gemv_mma_rows", w, None, x, bias, norm, residual, glu, w8=False,
                          single=False, kernel=kernel)


def plan_gemv_mma(N, K, w8=False, dtype=None):
    """The route of the ``kernel="mfma"`` products on ``[N, K]`` weights (rsvld_plan_gemv_mma, host only): ``_lib.GemvMmaPlan``.  There
    is no row count to pass: the route cannot depend on it."""
    pl = L.GemvMmaPlan()
    L.check(L.load().rsvld_plan_gemv_mma(int(N), int(K), int(bool(w8)), L.F16 if dtype is None else ops._DT[dtype], pl), "rsvld_plan_gemv_mma")
    return pl


def llama_decode_attention_rows(qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws=None, kernel="valu"):
    """``ops.llama_decode_attention`` for ``B`` sequences with a position each (rsvld_llama_decode_attention_rows): ``qkv [B, (n_q + 2 n_kv)
    * 128]``, ``cos`` / ``sin [B, 128]``, ``pos [B]`` DEVICE int64, caches ``[B, n_kv, max_len, 128]`` updated at ``pos[b]`` in sequence
    ``b``'s slice only; ``ws`` (optional, re-usable): fp32, ``B`` times the single workspace.  -> ``[B, n_q * 128]``.
    ``kernel="mfma"`` (opt-in, ``ops.DECODE_ATTENTION_KERNELS``): the attention on MFMAs (rsvld_llama_decode_attention_mma_rows,
    csrc/decode_attention.hip; launch name ``llama_decode_attention_mma_rows``), at every ``B`` including 1: the caches end bit for
    bit as "valu" leaves them, sequence ``b``'s output is bit-identical among ITS ``B``, ``max_len`` and neighbours, not to "valu" (fp32
    scores and a 16-bit P where "valu" has 16-bit scores and an fp32 P); ``ws``: ``decode_attention_ws_floats`` of the kernel."""
    return ops._decode_attention_rows("llama_decode_attention_rows", qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws, False, kernel)


def decode_attention_ws_floats(n_q, n_kv, max_len, B, kernel="valu"):
    """fp32 elements of the workspace one step of ``B`` sequences needs with ``kernel`` (rsvld_llama_decode_attention_rows_ws_bytes /
    rsvld_llama_decode_attention_mma_rows_ws_bytes): the one place that picks the symbol."""
    lib = L.load()
    ws_bytes = lib.rsvld_llama_decode_attention_mma_rows_ws_bytes if kernel == "mfma" else lib.rsvld_llama_decode_attention_rows_ws_bytes
    return int(ws_bytes(int(n_q), int(n_kv), int(max_len), int(B))) // 4


def plan_decode_attention_mma(n_q, n_kv, max_len, dtype=None):
    """The launch of the ``kernel="mfma"`` attention (rsvld_plan_llama_decode_attention_mma, host only): ``_lib.DecodeAttentionMmaPlan``.
    There is no sequence count to pass, and ``range_keys`` is the same for every ``max_len``."""
    pl = L.DecodeAttentionMmaPlan()
    L.check(L.load().rsvld_plan_llama_decode_attention_mma(int(n_q), int(n_kv), int(max_len), L.F16 if dtype is None else ops._DT[dtype], pl),
            "rsvld_plan_llama_decode_attention_mma")
    return pl
