"""The decode-step operators for SEVERAL independent sequences at once (rsvld_gemv_rows_fused, rsvld_gemv_w8_rows_fused,
rsvld_llama_decode_attention_rows): the batched token loop of the caption pass (``llava_next.FastDecoder(batch=B)``,
``infer_dir --caption_batch``), which streams the decoder's weights once per token for up to ``MAX_ROWS`` captions.

Contract: row ``b`` of every result is bit for bit what the single-row sibling (``ops.gemv_fused``, ``w8.gemv_w8``,
``ops.llama_decode_attention``) returns for row ``b`` alone, whatever ``B`` is and whatever the other rows hold
(tests/test_gpu_decode_rows.py compares with ``torch.equal``).  Operand contracts and errors are the siblings': every operand is
checked before anything is allocated or launched, a CPU tensor raises (there is no CPU path), launches go through ``ops._launch``."""
import torch

from . import _lib as L
from . import ops
from .ops import _HALF, _arg, _bad, _launch, _need_gpu, _ptr, _stream

MAX_ROWS = 8      # RSVLD_DECODE_MAX_ROWS


def _rows(fn, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        _bad(fn, "x", f"must be a [B, K] tensor of activation rows, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    B = x.shape[0]
    if not 1 <= B <= MAX_ROWS:
        _bad(fn, "x", f"has {B} rows, expected 1..{MAX_ROWS}")
    return B


def gemv_rows(w, x, bias=None, *, norm=None, residual=None, glu=False):
    """``ops.gemv_fused`` for ``B`` activation rows (rsvld_gemv_rows_fused): ``w [N, K]`` 16-bit, ``x [B, K]`` (``[B, 2 K]`` = gate | up
    with ``glu``), ``residual [B, N]``; ``bias [N]`` and ``norm=(weight [K], eps)`` are shared by the rows.  -> ``[B, N]``."""
    fn = "gemv_rows"
    _arg(fn, "w", w, _HALF, shape=(None, None))
    N, K = w.shape
    B = _rows(fn, x)
    nw, eps = (None, 0.0) if norm is None else norm
    _arg(fn, "x", x, w.dtype, shape=(B, 2 * K if glu else K))
    _arg(fn, "bias", bias, w.dtype, numel=N, optional=True)
    _arg(fn, "norm weight", nw, w.dtype, numel=x.shape[1], optional=True)
    _arg(fn, "residual", residual, w.dtype, shape=(B, N), optional=True)
    if glu and nw is not None:
        _bad(fn, "norm weight", "cannot be combined with glu")
    _need_gpu(w, x, bias, nw, residual)
    y = ops.torch.empty((B, N), device=w.device, dtype=w.dtype)
    lib = L.load()
    _launch(fn, 2.0 * B * N * K, (N * K + B * (K + N)) * 2, lambda: L.check(
        lib.rsvld_gemv_rows_fused(_ptr(w), _ptr(x), _ptr(bias), _ptr(nw), float(eps), _ptr(residual), int(glu), _ptr(y), N, K, B,
                                  ops._dt(w), _stream()), "rsvld_gemv_rows_fused"))
    return y


def gemv_w8_rows(q, scale, x, bias=None, *, norm=None, residual=None, glu=False):
    """``w8.gemv_w8`` for ``B`` activation rows (rsvld_gemv_w8_rows_fused): ``q [N, K]`` uint8 and ``scale [N]`` float32 from
    ``w8.pack_rows_e4m3``, ``x [B, K]`` 16-bit (``[B, 2 K]`` with ``glu``), ``residual [B, N]``.  -> ``[B, N]`` in ``x``'s type."""
    fn = "gemv_w8_rows"
    _arg(fn, "q", q, torch.uint8, shape=(None, None))
    N, K = q.shape
    if N == 0 or K == 0 or K % 16:
        _bad(fn, "q", f"has shape {tuple(q.shape)}: rows of whole 16-byte pieces of e4m3 (K % 16 == 0) expected")
    B = _rows(fn, x)
    nw, eps = (None, 0.0) if norm is None else norm
    _arg(fn, "scale", scale, torch.float32, numel=N)
    _arg(fn, "x", x, _HALF, shape=(B, 2 * K if glu else K))
    _arg(fn, "bias", bias, x.dtype, numel=N, optional=True)
    _arg(fn, "norm weight", nw, x.dtype, numel=x.shape[1], optional=True)
    _arg(fn, "residual", residual, x.dtype, shape=(B, N), optional=True)
    if glu and nw is not None:
        _bad(fn, "norm weight", "cannot be combined with glu")
    _need_gpu(q, scale, x, bias, nw, residual)
    y = ops.torch.empty((B, N), device=x.device, dtype=x.dtype)
    lib = L.load()
    _launch(fn, 2.0 * B * N * K, N * K + N * 4 + B * (K + N) * 2, lambda: L.check(
        lib.rsvld_gemv_w8_rows_fused(_ptr(q), _ptr(scale), _ptr(x), _ptr(bias), _ptr(nw), float(eps), _ptr(residual), int(glu), _ptr(y),
                                     N, K, B, ops._dt(x), _stream()), "rsvld_gemv_w8_rows_fused"))
    return y


def llama_decode_attention_rows(qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws=None):
    """``ops.llama_decode_attention`` for ``B`` sequences with a position each (rsvld_llama_decode_attention_rows): ``qkv [B, (n_q + 2 n_kv)
    * 128]``, ``cos`` / ``sin [B, 128]``, ``pos [B]`` DEVICE int64, caches ``[B, n_kv, max_len, 128]`` updated at ``pos[b]`` in sequence
    ``b``'s slice only; ``ws`` (optional, re-usable): fp32, ``B`` times the single workspace.  -> ``[B, n_q * 128]``."""
    fn = "llama_decode_attention_rows"
    _arg(fn, "kcache", kcache, _HALF, shape=(None, n_kv, None, None))
    B, hd, max_len = kcache.shape[0], kcache.shape[-1], kcache.shape[-2]
    if not 1 <= B <= MAX_ROWS:
        _bad(fn, "kcache", f"holds {B} sequences, expected 1..{MAX_ROWS}")
    _arg(fn, "vcache", vcache, kcache.dtype, shape=tuple(kcache.shape))
    _arg(fn, "qkv", qkv, kcache.dtype, shape=(B, (n_q + 2 * n_kv) * hd))
    _arg(fn, "cos", cos, kcache.dtype, shape=(B, hd))
    _arg(fn, "sin", sin, kcache.dtype, shape=(B, hd))
    _arg(fn, "pos", pos, torch.int64, shape=(B,))
    _arg(fn, "ws", ws, torch.float32, shape=(None,), optional=True)
    _need_gpu(qkv, cos, sin, pos, kcache, vcache, ws)
    lib = L.load()
    ws_n = int(lib.rsvld_llama_decode_attention_rows_ws_bytes(n_q, n_kv, max_len, B)) // 4
    if ws is None:
        ws = ops.torch.empty(ws_n, device=qkv.device, dtype=torch.float32)
    elif ws.numel() < ws_n:
        _bad(fn, "ws", f"has {ws.numel()} fp32 elements, the step needs {ws_n}")
    out = ops.torch.empty((B, n_q * hd), device=qkv.device, dtype=qkv.dtype)
    _launch(fn, 0.0, 0.0, lambda: L.check(
        lib.rsvld_llama_decode_attention_rows(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(kcache), _ptr(vcache), _ptr(out), _ptr(ws),
                                              n_q, n_kv, hd, max_len, B, float(scale), ops._dt(qkv), _stream()),
        "rsvld_llama_decode_attention_rows"))
    return out
