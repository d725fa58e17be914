"""Products on OCP e4m3 weights with one power-of-two scale per output row (rsvld_pack_rows_e4m3, rsvld_gemv_w8_fused, rsvld_gemm_w8):
the opt-in ``weights="e4m3"`` mode of the caption pass's token loop (``llava_next.FastDecoder``), which is bound by weight bytes alone,
and -- ``prefill_weights="e4m3"`` -- the prefill's projections on the same bytes (``linear_w8``: a tile GEMM, many activation rows).

The quantiser, exactly (``pack_rows_e4m3_host`` is this paragraph in torch, bit for bit what the kernel writes): for a 16-bit row
``w[n, :]`` take ``amax`` over its finite elements; ``e[n]`` is the smallest integer with ``amax * 2^-e <= 448``, computed from
``amax = m * 2^x`` (``frexp``, ``m`` in [0.5, 1)) and ``448 = 0.875 * 2^9`` as ``e = x - 9`` if ``m <= 0.875`` else ``x - 8``; 0 for an
all-zero row; clamped to [-126, 127].  ``q[n, k] = e4m3_rne(w[n, k] * 2^-e[n])``: the scaling is exact and nothing saturates.  A
non-finite weight becomes byte 0x7F (e4m3 NaN), so a corrupt checkpoint shows as NaN logits.  Storage: ``q`` uint8 ``[N, K]``
(``K % 16 == 0``: 16-byte rows), ``scale`` float32 ``[N]`` = ``2^e``.

Like every wrapper of ``ops``, the device functions check their operands before anything is allocated or launched, raise on a CPU
tensor (there is no CPU path) and launch through ``ops._launch`` so the profiler sees them."""
import torch

from . import _lib as L
from . import ops
from .ops import _HALF, _arg, _bad, _launch, _need_gpu, _ptr, _stream

E4M3_NAN = 0x7F


def pack_rows_e4m3(w):
    """16-bit ``w [N, K]`` (contiguous, ``K % 16 == 0``) -> ``(q uint8 [N, K], scale float32 [N])`` on the device (rsvld_pack_rows_e4m3)."""
    _arg("pack_rows_e4m3", "w", w, _HALF, shape=(None, None))
    N, K = w.shape
    if N == 0 or K == 0 or K % 16:
        _bad("pack_rows_e4m3", "w", f"has shape {tuple(w.shape)}: rows of whole 16-byte pieces of e4m3 (K % 16 == 0) expected")
    _need_gpu(w)
    q = ops.torch.empty((N, K), device=w.device, dtype=torch.uint8)        # (through ``ops.torch``, like every output of ops.py)
    scale = ops.torch.empty(N, device=w.device, dtype=torch.float32)
    lib = L.load()
    _launch("pack_rows_e4m3", 0.0, N * K * 3 + N * 4, lambda: L.check(
        lib.rsvld_pack_rows_e4m3(_ptr(w), _ptr(q), _ptr(scale), N, K, ops._dt(w), _stream()), "rsvld_pack_rows_e4m3"))
    return q, scale


def gemv_w8(q, scale, x, bias=None, *, norm=None, residual=None, glu=False):
    """``ops.gemv_fused`` on packed weights (rsvld_gemv_w8_fused): ``q [N, K]`` uint8 and ``scale [N]`` float32 from ``pack_rows_e4m3``,
    ONE 16-bit activation row ``x`` (``[K]``, or ``[2 K]`` = gate | up with ``glu``) -> ``T(scale * (q x') + bias)``, then the residual,
    in ``x``'s type.  ``norm`` / ``glu`` / ``residual`` as in ``ops.gemv_fused``, with its roundings."""
    return ops._gemv_rows("gemv_w8", "gemv_w8", q, scale, x, bias, norm, residual, glu, w8=True, single=True)


def gemv_w8_rows(q, scale, x, bias=None, *, norm=None, residual=None, glu=False, kernel="valu"):
    """``gemv_w8`` for ``B`` activation rows (rsvld_gemv_w8_rows_fused; also ``decode_rows.gemv_w8_rows``): ``x [B, K]`` 16-bit
    (``[B, 2 K]`` with ``glu``), ``residual [B, N]``; ``bias`` and ``norm`` are shared by the rows.  -> ``[B, N]`` in ``x``'s type.
    ``kernel="mfma"`` (opt-in): rsvld_gemv_w8_mma_rows_fused, as ``decode_rows.gemv_rows`` describes it."""
    return ops._gemv_rows("gemv_w8_rows", "gemv_w8_rows" if kernel == "valu" else "gemv_w8_mma_rows", q, scale, x, bias, norm, residual, glu,
                          w8=True, single=False, kernel=kernel)


def linear_w8(q, scale, x, bias=None):
    """``torch.nn.functional.linear`` on packed weights for ``M`` activation rows (rsvld_gemm_w8): ``q [N, K]`` uint8 and ``scale [N]``
    float32 from ``pack_rows_e4m3``, ``x [M, K]`` 16-bit with contiguous rows, ``bias [N]`` in ``x``'s type or None ->
    ``T(scale * (x q^T) + bias)`` as ``[M, N]`` in ``x``'s type.  A tile GEMM on 16-bit MFMAs (the bytes are converted unscaled, the
    scale meets the fp32 sum); row ``m`` of the result depends on row ``m`` of ``x`` alone, bit for bit, whatever ``M`` is."""
    fn = "linear_w8"
    _arg(fn, "q", q, torch.uint8, shape=(None, None))
    N, K = q.shape
    if N == 0 or K == 0 or K % 16:
        _bad(fn, "q", f"has shape {tuple(q.shape)}: rows of whole 16-byte pieces of e4m3 (K % 16 == 0) expected")
    _arg(fn, "scale", scale, torch.float32, numel=N)
    _arg(fn, "x", x, _HALF, shape=(None, K))
    M = x.shape[0]
    if M == 0:
        _bad(fn, "x", "has no rows")
    _arg(fn, "bias", bias, x.dtype, numel=N, optional=True)
    _need_gpu(q, scale, x, bias)
    out = ops.torch.empty((M, N), device=x.device, dtype=x.dtype)
    lib = L.load()
    _launch(fn, 2.0 * M * N * K, N * K + N * 4 + M * (K + N) * 2, lambda: L.check(
        lib.rsvld_gemm_w8(_ptr(x), _ptr(q), _ptr(scale), _ptr(bias), _ptr(out), M, N, K, ops._dt(x), _stream()), "rsvld_gemm_w8"))
    return out


def plan_linear(M, N, K, dtype=torch.float16):
    """The launch of ``linear_w8`` on such shapes (rsvld_plan_gemm_w8, host only): ``_lib.GemmW8Plan``.  ``M`` enters ``grid_x`` alone."""
    pl = L.GemmW8Plan()
    L.check(L.load().rsvld_plan_gemm_w8(int(M), int(N), int(K), ops._DT[dtype], pl), "rsvld_plan_gemm_w8")
    return pl


# ----------------------------------------------------------------------------- host model (what the tests compare the kernels with)
def row_exponents_host(w):
    """``e [N]`` (int32) of the rule above, from ``torch.frexp``."""
    wf = w.detach().to(device="cpu", dtype=torch.float32)
    amax = torch.where(torch.isfinite(wf), wf.abs(), torch.zeros(())).amax(dim=1)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    return torch.where(amax == 0, torch.zeros_like(e), e).clamp(-126, 127).to(torch.int32)


def pack_rows_e4m3_host(w):
    """The quantiser on the host: 16-bit ``w [N, K]`` -> ``(q uint8 [N, K], scale float32 [N])`` on the CPU.  torch's cast to
    ``float8_e4m3fn`` rounds to nearest even, as the hardware conversion does."""
    wf = w.detach().to(device="cpu", dtype=torch.float32)
    e = row_exponents_host(w)
    one = torch.ones(e.shape, dtype=torch.float32)
    q = (wf * torch.ldexp(one, -e)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    q[~torch.isfinite(wf)] = E4M3_NAN
    return q, torch.ldexp(one, e)


def dequant(q, scale):
    """``(q, scale)`` -> the float32 ``[N, K]`` the kernel multiplies with: exact (e4m3 has 4 significant bits, the scale is a power of
    two)."""
    return q.view(torch.float8_e4m3fn).to(torch.float32) * scale.to(torch.float32)[:, None]
