"""The image steps around the two stages on the GPU (csrc/image.hip): Pillow's 8-bit bicubic resize, the uint8 <-> fp32 converters
and ATen's fp32 bicubic fused with the 8-bit quantiser.  Opt-in (``PipelineConfig.device_io``); the host functions they mirror --
``data.dataset.load_sr_input``, ``utils.tensor2img.tensor2img``, ``models.util.PIL2Tensor`` / ``Tensor2PIL`` -- stay the default.

Everything that decides a bit is computed HERE, on the host, and handed to the kernels as small device tables: the filter
coefficients and bounds of Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` (float64, same order of operations), the two
256-entry look-up tables (the host functions' very expressions on ``arange(256)``) and ATen's bicubic tap indices and weights (fp32).
The kernels only gather, multiply-accumulate and store, so the resize, both converters and ``tensor2img`` equal the host route bit
for bit; the fp32 bicubic of ``Tensor2PIL`` sums its taps in a fixed order that is not ATen's vectorised one and differs from it by
one 8-bit step in a few bytes per 100 000.  The caption's views (``caption_views``: ``llava_next.process_anyres_image`` of the device
hand-off image) follow the same rule: the two Pillow resizes, then one gather through a 3 x 256 table that is read off the CLIP image
processor itself (``clip_lut``), bit for bit the host route's views.

Same rules as ``ops.py``: operand contracts through ``ops._arg``, outputs through ``ops.torch``, launches through ``ops._launch`` on
the current stream, no CPU fallback, no mutable module global.  Tables are cached on an ``ImagePlan`` its user owns."""
import numpy as np
import torch as _torch

from . import _lib as L
from . import ops as O
from .data.dataset import resize_geometry
from .models.util import pil2tensor_size

PRECISION_BITS = 32 - 8 - 2          # Pillow's fixed point (src/libImaging/Resample.c)
MODE_TENSOR2IMG, MODE_TENSOR2PIL = 0, 1


# ----------------------------------------------------------------------------- host tables (numpy; no GPU)
def _pillow_bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def pillow_bicubic_table(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the BICUBIC filter over the whole axis, in float64 with Pillow's
    order of operations -> ``(bounds int32 [out, 2] = (xmin, n), coeffs int32 [out, ksize])``; taps past ``n`` are 0."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise L.RsvldError(f"pillow_bicubic_table: sizes must be positive, got {in_size} -> {out_size}")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, _pillow_bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]          # summed left to right (cumsum is sequential); the dead taps add +0.0
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = np.trunc(np.where(w < 0, -0.5, 0.5) + w * (1 << PRECISION_BITS)).astype(np.int32)
    fixed[~live] = 0
    return np.stack([xmin, n], axis=1).astype(np.int32), fixed


def identity_table(size):
    """``(bounds, coeffs)`` of the pass that copies: output j = source j, weight 1 << PRECISION_BITS."""
    j = np.arange(int(size), dtype=np.int32)
    return np.stack([j, np.ones_like(j)], axis=1), np.full((int(size), 1), 1 << PRECISION_BITS, np.int32)


def apply_pillow_table(src, table, axis, first=0, out_len=None):
    """One pass of the 8-bit resize in numpy integer arithmetic (the kernel's arithmetic; CPU tests and documentation).
    ``axis`` 0 = horizontal, 1 = vertical, as ``resample_u8``."""
    bounds, coeffs = table
    out_len = bounds.shape[0] - first if out_len is None else out_len
    s = np.moveaxis(np.asarray(src), 1 - axis, 0).astype(np.int64)          # resampled axis first
    out = np.empty((out_len,) + s.shape[1:], np.uint8)
    for j in range(out_len):
        lo, n = (int(v) for v in bounds[first + j])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coeffs[first + j, :n].astype(np.int64), s[lo:lo + n], axes=1)
        out[j] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, 1 - axis)


def pillow_resize_numpy(src, size, box=None):
    """``Image.resize(size, BICUBIC)`` of an HWC uint8 array, restated: horizontal pass, then vertical, a pass whose size does not
    change skipped.  ``box`` = (left, top, width, height) of the result to keep (the loader's centre crop)."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    nw, nh = size
    left, top, bw, bh = (0, 0, nw, nh) if box is None else box
    if nw != w:
        src = apply_pillow_table(src, pillow_bicubic_table(w, nw), 0, left, bw)
    else:
        src = src[:, left:left + bw]
    if nh != h:
        src = apply_pillow_table(src, pillow_bicubic_table(h, nh), 1, top, bh)
    else:
        src = src[top:top + bh]
    return np.ascontiguousarray(src)


def stage2_lut():
    """``PIL2Tensor``'s ``x / 255 * 2 - 1`` (float64, then fp32) for the 256 byte values."""
    x = np.arange(256).astype(np.uint8)
    x = x / 255 * 2 - 1
    return _torch.tensor(x, dtype=_torch.float32).numpy()


def loader_lut():
    """``load_sr_input``'s ``((x.float() / 255.0) - 0.5) / 0.5`` (fp32 torch) for the 256 byte values."""
    x = _torch.from_numpy(np.arange(256).astype(np.uint8)).float() / 255.0
    return ((x - 0.5) / 0.5).numpy()


def aten_bicubic_table(in_size, out_size):
    """ATen's ``upsample_bicubic2d`` tables for one axis (align_corners=False, A = -0.75), in fp32 as ATen computes them
    -> ``(idx int32 [out, 4] clamped to [0, in - 1], w fp32 [out, 4])``."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise L.RsvldError(f"aten_bicubic_table: sizes must be positive, got {in_size} -> {out_size}")
    f = np.float32
    A = f(-0.75)
    s = f(in_size) / f(out_size)
    real = s * (np.arange(out_size, dtype=f) + f(0.5)) - f(0.5)
    i0 = np.floor(real)
    t = np.minimum(np.maximum(real - i0, f(0)), f(1))

    def c1(x):
        return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

    def c2(x):
        return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A

    x2 = f(1) - t
    w = np.stack([c2(t + f(1)), c1(t), c1(x2), c2(x2 + f(1))], axis=1).astype(f)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, in_size - 1).astype(np.int32)
    return idx, w


def quantise_numpy(x, mode):
    """The two 8-bit quantisers on an fp32 array (the kernel's arithmetic: every product and sum rounded to fp32 on its own)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    if mode == MODE_TENSOR2IMG:
        return np.round((np.clip(x, f(-1), f(1)) + f(1)) * f(0.5) * f(255)).astype(np.uint8)
    return np.clip(x * f(127.5) + f(127.5), f(0), f(255)).astype(np.uint8)


def bicubic_quantise_numpy(x, h0, w0):
    """``rsvld_bicubic_f32_to_u8_hwc`` in numpy fp32: ``x`` [C, H, W] -> uint8 [h0, w0, C], the kernel's summation order."""
    x = np.asarray(x, dtype=np.float32)
    (iy, wy), (ix, wx) = aten_bicubic_table(x.shape[1], h0), aten_bicubic_table(x.shape[2], w0)
    v = None
    for i in range(4):
        rows = x[:, iy[:, i], :]                                        # [C, h0, W]
        t = wx[None, None, :, 0] * rows[:, :, ix[:, 0]]
        for j in range(1, 4):
            t = t + wx[None, None, :, j] * rows[:, :, ix[:, j]]
        v = wy[None, :, None, i] * t if v is None else v + wy[None, :, None, i] * t
    return quantise_numpy(v, MODE_TENSOR2PIL).transpose(1, 2, 0)


# ----------------------------------------------------------------------------- the caption's views (host side; no GPU)
def anyres_layout(image_size, edge, grid_pinpoints):
    """Where ``llava_next.process_anyres_image`` puts an image of ``image_size`` = (width, height) for tiles of ``edge`` pixels ->
    ``(tw, th, nw, nh, ox, oy)``: the canvas, the aspect-preserving size and the paste offset (``llava_next``'s own arithmetic)."""
    from . import llava_next as LN
    size = (int(image_size[0]), int(image_size[1]))
    tw, th = LN.select_best_resolution(size, LN._resolutions(grid_pinpoints, edge))
    return (tw, th) + LN.fit_and_offset(size, (tw, th))


def _clip_probe(S, shuffled):
    """S x S RGB probe: every channel takes all 256 byte values (a ramp over the pixels in row-major order, or -- ``shuffled`` -- the
    ramp in a fixed seeded order), each channel another byte at the same pixel."""
    ramp = np.arange(S * S, dtype=np.int64)
    if shuffled:
        ramp = np.random.default_rng(0).permutation(ramp)
    ramp = ramp.reshape(S, S)
    return np.ascontiguousarray(np.stack([(ramp + 85 * c) % 256 for c in range(3)], axis=2).astype(np.uint8))


def clip_lut(processor, dtype=_torch.float32):
    """What ``processor.preprocess`` does to a byte of an S x S RGB image, MEASURED: a host ``[3, 256]`` table of ``dtype`` read off
    the processor's own result on a probe image (so it holds whatever the installed transformers computes: rescale in fp32 or fp64,
    either backend), ``table[c][byte]``; 16-bit tables are the fp32 table rounded, as the host route's ``.to(dtype)`` rounds the views.
    Raises ``RsvldError`` where the processor is not such a table at S x S (it resizes, crops or flips there, or returns another
    shape), where its resize edge and crop differ, and for S * S < 256 (the probe cannot hold every byte)."""
    from PIL import Image
    from . import llava_next as LN
    edge, crop = LN._proc_sizes(processor)
    if edge != crop:
        raise L.RsvldError(f"clip_lut: the processor resizes to {edge} and crops to {crop}: its tiles are not taken pixel for pixel")
    S = edge
    if S * S < 256:
        raise L.RsvldError(f"clip_lut: a {S} x {S} probe cannot hold all 256 byte values")

    def run(probe):
        out = processor.preprocess(Image.fromarray(probe), return_tensors="pt")["pixel_values"]
        if tuple(out.shape) != (1, 3, S, S) or out.dtype != _torch.float32:
            raise L.RsvldError(f"clip_lut: preprocess of a {S} x {S} image gave {tuple(out.shape)} {out.dtype}, expected (1, 3, {S}, {S}) fp32")
        return out[0].numpy().view(np.int32).reshape(3, -1)          # compared as bits

    probe = _clip_probe(S, False)
    bits = run(probe)
    table = np.zeros((3, 256), np.int32)
    for c in range(3):
        table[c, probe[..., c].reshape(-1)] = bits[c]
    # one value per byte, wherever the byte stands: on the probe itself, and on the shuffled probe (where S * S = 256 leaves a
    # single pixel per byte, only the second image shows a processor that moves pixels)
    for p, got in ((probe, bits), (_clip_probe(S, True), None)):
        got = run(p) if got is None else got
        for c in range(3):
            if not np.array_equal(table[c, p[..., c].reshape(-1)], got[c]):
                raise L.RsvldError(f"clip_lut: preprocess is not a per-byte table at {S} x {S} (channel {c}: one byte, two values): "
                                   "it resizes, crops or flips there")
    return _torch.from_numpy(table.view(np.float32)).to(dtype)


def assemble_views_numpy(whole, fit, lut, layout):
    """``rsvld_clip_views_u8`` in numpy: ``whole`` [S, S, 3] and ``fit`` [nh, nw, 3] uint8, ``lut`` [3, 256], ``layout`` of
    ``anyres_layout`` -> [1 + tiles, 3, S, S] of the table's type (view 0 the squashed image, then the canvas's tiles row by row)."""
    tw, th, nw, nh, ox, oy = layout
    S = whole.shape[0]
    canvas = np.zeros((th, tw, 3), np.uint8)
    canvas[oy:oy + nh, ox:ox + nw] = fit
    views = [whole] + [canvas[y:y + S, x:x + S] for y in range(0, th, S) for x in range(0, tw, S)]
    lut = np.asarray(lut)
    return np.stack([np.stack([lut[c][v[..., c]] for c in range(3)], axis=0) for v in views], axis=0)


def caption_views_numpy(u8, processor, grid_pinpoints):
    """``llava_next.process_anyres_image`` of the HWC uint8 RGB array ``u8``, restated (CPU tests and documentation): Pillow's resize
    to the fitted size and to S x S (``pillow_resize_numpy``), the fitted image on a black canvas, the canvas's S x S tiles row by
    row, every byte through ``clip_lut`` -> fp32 [1 + tiles, 3, S, S], equal to the host function bit for bit."""
    from . import llava_next as LN
    u8 = np.asarray(u8)
    S = LN._proc_sizes(processor)[0]
    layout = anyres_layout((u8.shape[1], u8.shape[0]), S, grid_pinpoints)
    fit = pillow_resize_numpy(u8, layout[2:4])
    return assemble_views_numpy(pillow_resize_numpy(u8, (S, S)), fit, clip_lut(processor).numpy(), layout)


# ----------------------------------------------------------------------------- device tables
class ImagePlan:
    """The device tables of one user (a pipeline, a benchmark), cached per ``(kind, in, out, device)``.  Building a table is host
    arithmetic plus one small upload; a pipeline meets the same few sizes for every image."""

    def __init__(self):
        self._tables = {}

    def _get(self, key, build):
        if key not in self._tables:
            self._tables[key] = build()
        return self._tables[key]

    def pillow(self, in_size, out_size, device):
        device = _torch.device(device)
        return self._get(("pillow", in_size, out_size, device),
                         lambda: tuple(_torch.from_numpy(a).to(device) for a in pillow_bicubic_table(in_size, out_size)))

    def aten(self, in_size, out_size, device):
        device = _torch.device(device)
        return self._get(("aten", in_size, out_size, device),
                         lambda: tuple(_torch.from_numpy(a).to(device) for a in aten_bicubic_table(in_size, out_size)))

    def identity(self, size, device):
        """The table of a pass that changes no size (a crop in that axis, or the copy of a resize to the same size): one tap of weight
        1.0 per output, which the fixed-point arithmetic reproduces exactly."""
        device = _torch.device(device)
        return self._get(("identity", size, size, device),
                         lambda: tuple(_torch.from_numpy(a).to(device) for a in identity_table(size)))

    def lut(self, kind, device):
        device = _torch.device(device)
        build = {"stage2": stage2_lut, "loader": loader_lut}[kind]
        return self._get(("lut", kind, device), lambda: _torch.from_numpy(build()).to(device))

    def clip_lut(self, processor, dtype, device):
        """``clip_lut(processor, dtype)`` on ``device``, measured once per processor setting (not per processor object)."""
        from . import llava_next as LN
        device = _torch.device(device)
        flags = tuple(getattr(processor, f, None) for f in ("do_resize", "do_center_crop", "do_rescale", "do_normalize", "do_convert_rgb"))
        mean, std = (None if v is None else tuple(float(x) for x in v) for v in (processor.image_mean, processor.image_std))
        key = ("clip", mean, std, getattr(processor, "rescale_factor", None), flags, LN._proc_sizes(processor), dtype, device)
        return self._get(key, lambda: clip_lut(processor, dtype).to(device))


# ----------------------------------------------------------------------------- launching wrappers
def _image_u8(fn, name, t):
    O._arg(fn, name, t, _torch.uint8, shape=(None, None, None))
    if not 1 <= t.shape[2] <= 4 or t.shape[0] == 0 or t.shape[1] == 0:
        O._bad(fn, name, f"must be a non-empty HWC image of 1..4 channels, got shape {tuple(t.shape)}")
    return t


def _image_f32(fn, name, t):
    O._arg(fn, name, t, _torch.float32, shape=(None, None, None))
    if not 1 <= t.shape[0] <= 4 or t.shape[1] == 0 or t.shape[2] == 0:
        O._bad(fn, name, f"must be a non-empty CHW image of 1..4 channels, got shape {tuple(t.shape)}")
    return t


def resample_u8(src, table, axis, first=0, out_len=None):
    """One pass of Pillow's 8-bit bicubic resize over HWC uint8 ``src``.  ``axis`` 0: horizontal -> [H, out_len, C]; 1: vertical ->
    [out_len, W, C].  ``table``: ``ImagePlan.pillow(in, out, device)``; output j uses its row ``first + j``."""
    fn = "resample_u8"
    _image_u8(fn, "src", src)
    if axis not in (0, 1):
        raise L.RsvldOperandError(f"{fn}: axis must be 0 (horizontal) or 1 (vertical), got {axis!r}")
    if not isinstance(table, (tuple, list)) or len(table) != 2:
        raise L.RsvldOperandError(f"{fn}: table must be the (bounds, coeffs) pair of ImagePlan.pillow")
    bounds, coeffs = table
    O._arg(fn, "table[0]", bounds, _torch.int32, shape=(None, 2))
    O._arg(fn, "table[1]", coeffs, _torch.int32, shape=(bounds.shape[0], None))
    rows, ksize = coeffs.shape
    out_len = rows - first if out_len is None else out_len
    if first < 0 or out_len <= 0 or first + out_len > rows or ksize == 0:
        O._bad(fn, "table[0]", f"has {rows} rows: the outputs [{first}, {first + out_len}) do not fit")
    H, W, Cc = src.shape
    O._need_gpu(src, bounds, coeffs)
    out = O.torch.empty((H, out_len, Cc) if axis == 0 else (out_len, W, Cc), device=src.device, dtype=_torch.uint8)
    O._launch(f"resample_u8_{'hv'[axis]}", 2.0 * out.numel() * ksize, src.numel() + out.numel(), lambda: L.check(
        L.load().rsvld_resample_u8(O._ptr(src), O._ptr(out), O._ptr(bounds), O._ptr(coeffs), H, W, Cc, axis, out_len, first,
                                   rows, ksize, O._stream()), "rsvld_resample_u8"))
    return out


def u8_to_nchw_f32(src, lut):
    """HWC uint8 -> fp32 [C, H, W] through the 256-entry table ``lut`` (``ImagePlan.lut``)."""
    fn = "u8_to_nchw_f32"
    _image_u8(fn, "src", src)
    O._arg(fn, "lut", lut, _torch.float32, shape=(256,))
    O._need_gpu(src, lut)
    H, W, Cc = src.shape
    out = O.torch.empty((Cc, H, W), device=src.device, dtype=_torch.float32)
    O._launch("u8_hwc_to_nchw_f32", 0.0, 5.0 * src.numel(), lambda: L.check(
        L.load().rsvld_u8_hwc_to_nchw_f32(O._ptr(src), O._ptr(lut), O._ptr(out), H, W, Cc, O._stream()),
        "rsvld_u8_hwc_to_nchw_f32"))
    return out


def nchw_f32_to_u8(x, mode):
    """fp32 [C, H, W] -> HWC uint8; ``mode``: MODE_TENSOR2IMG (clamp to [-1, 1], round) or MODE_TENSOR2PIL (x127.5+127.5, truncate)."""
    fn = "nchw_f32_to_u8"
    _image_f32(fn, "x", x)
    if mode not in (MODE_TENSOR2IMG, MODE_TENSOR2PIL):
        raise L.RsvldOperandError(f"{fn}: unknown mode {mode!r}")
    O._need_gpu(x)
    Cc, H, W = x.shape
    out = O.torch.empty((H, W, Cc), device=x.device, dtype=_torch.uint8)
    O._launch("nchw_f32_to_u8_hwc", 0.0, 5.0 * x.numel(), lambda: L.check(
        L.load().rsvld_nchw_f32_to_u8_hwc(O._ptr(x), O._ptr(out), H, W, Cc, mode, O._stream()), "rsvld_nchw_f32_to_u8_hwc"))
    return out


def bicubic_f32_to_u8(x, table_y, table_x):
    """``F.interpolate(mode="bicubic")`` of fp32 [C, H, W] to ``(len(table_y), len(table_x))``, quantised as ``Tensor2PIL`` -> HWC
    uint8.  ``table_*``: ``ImagePlan.aten(in, out, device)`` of the axis."""
    fn = "bicubic_f32_to_u8"
    _image_f32(fn, "x", x)
    for name, tab in (("table_y", table_y), ("table_x", table_x)):
        if not isinstance(tab, (tuple, list)) or len(tab) != 2:
            raise L.RsvldOperandError(f"{fn}: {name} must be the (idx, w) pair of ImagePlan.aten")
        O._arg(fn, name + "[0]", tab[0], _torch.int32, shape=(None, 4))
        O._arg(fn, name + "[1]", tab[1], _torch.float32, shape=(tab[0].shape[0], 4))
        if tab[0].shape[0] == 0:
            O._bad(fn, name + "[0]", "is empty")
    O._need_gpu(x, *table_y, *table_x)
    Cc, H, W = x.shape
    h0, w0 = table_y[0].shape[0], table_x[0].shape[0]
    out = O.torch.empty((h0, w0, Cc), device=x.device, dtype=_torch.uint8)
    O._launch("bicubic_f32_to_u8_hwc", 32.0 * out.numel(), 4.0 * x.numel() + out.numel(), lambda: L.check(
        L.load().rsvld_bicubic_f32_to_u8_hwc(O._ptr(x), O._ptr(out), O._ptr(table_y[0]), O._ptr(table_y[1]), O._ptr(table_x[0]),
                                             O._ptr(table_x[1]), Cc, H, W, h0, w0, O._stream()), "rsvld_bicubic_f32_to_u8_hwc"))
    return out


_VIEW_DT = {_torch.float16: L.F16, _torch.bfloat16: L.BF16, _torch.float32: L.F32}


def clip_views(whole, fit, lut, layout, dtype=_torch.float16):
    """The caption's views from its two resized images: ``whole`` uint8 [S, S, 3] (the image squashed to S x S), ``fit`` uint8
    [nh, nw, 3] (the aspect-preserving resize), ``lut`` [3, 256] of ``dtype`` (``ImagePlan.clip_lut``), ``layout`` = (tw, th, nw, nh,
    ox, oy) of ``anyres_layout`` -> ``dtype`` [1 + tiles, 3, S, S]: view 0 is ``whole``, the others the S x S tiles, row by row, of the
    black tw x th canvas that holds ``fit`` at (ox, oy); every byte through its channel's table."""
    fn = "clip_views"
    _image_u8(fn, "whole", whole)
    _image_u8(fn, "fit", fit)
    if dtype not in _VIEW_DT:
        raise L.RsvldOperandError(f"{fn}: dtype must be one of {tuple(_VIEW_DT)}, got {dtype!r}")
    S = whole.shape[0]
    O._arg(fn, "whole", whole, _torch.uint8, shape=(S, S, 3))
    O._arg(fn, "lut", lut, dtype, shape=(3, 256))
    try:
        tw, th, nw, nh, ox, oy = (int(v) for v in layout)
    except (TypeError, ValueError):
        raise L.RsvldOperandError(f"{fn}: layout must be the (tw, th, nw, nh, ox, oy) of anyres_layout, got {layout!r}") from None
    O._arg(fn, "fit", fit, _torch.uint8, shape=(nh, nw, 3))
    if tw <= 0 or th <= 0 or tw % S or th % S or ox < 0 or oy < 0 or ox + nw > tw or oy + nh > th:
        raise L.RsvldOperandError(f"{fn}: layout {(tw, th, nw, nh, ox, oy)}: the canvas must be whole tiles of {S} and hold the image")
    O._need_gpu(whole, fit, lut)
    gx, gy = tw // S, th // S
    out = O.torch.empty((1 + gx * gy, 3, S, S), device=whole.device, dtype=dtype)
    O._launch("clip_views_u8", 0.0, whole.numel() + fit.numel() + out.numel() * out.element_size(), lambda: L.check(
        L.load().rsvld_clip_views_u8(O._ptr(whole), O._ptr(fit), O._ptr(lut), O._ptr(out), S, nw, nh, ox, oy, gx, gy, _VIEW_DT[dtype],
                                     O._stream()), "rsvld_clip_views_u8"))
    return out


# ----------------------------------------------------------------------------- the host functions' device mirrors
def resize_u8(src, size, plan=None, box=None):
    """``Image.resize(size, BICUBIC)`` of HWC uint8 ``src`` on the device: Pillow's horizontal pass, then its vertical pass, each with a
    uint8 intermediate; a pass whose size does not change is skipped, or runs on the identity table where it has to crop or copy.
    ``box`` = (left, top, width, height): only that window of the result is computed (``Image.crop`` after the resize)."""
    _image_u8("resize_u8", "src", src)
    plan = ImagePlan() if plan is None else plan
    H, W, _ = src.shape
    nw, nh = (int(v) for v in size)
    left, top, bw, bh = (0, 0, nw, nh) if box is None else (int(v) for v in box)
    if nw <= 0 or nh <= 0 or left < 0 or top < 0 or bw <= 0 or bh <= 0 or left + bw > nw or top + bh > nh:
        raise L.RsvldOperandError(f"resize_u8: the window {(left, top, bw, bh)} does not fit the size {(nw, nh)}")
    O._need_gpu(src)
    out = src
    if nw != W or left or bw != W:
        out = resample_u8(out, plan.pillow(W, nw, src.device) if nw != W else plan.identity(W, src.device), 0, left, bw)
    if nh != H or top or bh != H or out is src:
        out = resample_u8(out, plan.pillow(H, nh, src.device) if nh != H else plan.identity(H, src.device), 1, top, bh)
    return out


def upload_u8(img, device):
    """A decoded RGB image (PIL or array) -> device uint8 HWC."""
    arr = np.array(img, dtype=np.uint8)          # (a copy: PIL's buffer is read-only)
    if arr.ndim != 3:
        raise L.RsvldOperandError(f"an RGB image is expected, got an array of shape {arr.shape}")
    host = _torch.from_numpy(np.ascontiguousarray(arr))
    if _torch.device(device).type != "cuda":
        return host.to(device)
    # from pinned memory, queued like a kernel: an upload from pageable memory makes the host wait for everything that is queued on
    # the current stream (the pinned block is the host allocator's: it is not handed out again before the copy has run)
    return host.pin_memory().to(device, non_blocking=True)


def load_sr_input(image, scale=1, device="cuda:0", plan=None):
    """``data.dataset.load_sr_input`` with the resize, the centre crop and the conversion on the device: ``image`` is a path or a PIL
    image (decoded on the host, uploaded as uint8) -> {'SR': fp32 [1, 3, S, S] on ``device``, 'Index': tensor([0])}."""
    from PIL import Image
    plan = ImagePlan() if plan is None else plan
    img = image if isinstance(image, Image.Image) else Image.open(image)
    src = upload_u8(img.convert("RGB"), device)
    nw, nh, target, left, top = resize_geometry(src.shape[1], src.shape[0], scale)
    sq = resize_u8(src, (nw, nh), plan, box=(left, top, target, target))
    return {"SR": u8_to_nchw_f32(sq, plan.lut("loader", src.device)).unsqueeze(0), "Index": _torch.tensor([0])}


def tensor2img(tensor, min_max=(-1, 1)):
    """``utils.tensor2img.tensor2img`` (uint8 output) of an fp32 ``[3, H, W]`` / ``[1, 3, H, W]`` device tensor -> device uint8 HWC.
    Only ``min_max = (-1, 1)``: the kernel's arithmetic is that range's."""
    if tuple(min_max) != (-1, 1):
        raise L.RsvldError(f"imageops.tensor2img: only min_max = (-1, 1) has a kernel, got {min_max!r}")
    if isinstance(tensor, _torch.Tensor) and tensor.dim() == 4 and tensor.shape[0] == 1:
        tensor = tensor[0]
    return nchw_f32_to_u8(tensor, MODE_TENSOR2IMG)


def pil2tensor(u8, upscale=1, min_size=1024, fix_resize=None, plan=None):
    """``models.util.PIL2Tensor`` of a device HWC uint8 image -> (fp32 [3, H, W] on the device, h0, w0)."""
    _image_u8("pil2tensor", "u8", u8)
    plan = ImagePlan() if plan is None else plan
    w, h, h0, w0 = pil2tensor_size(u8.shape[1], u8.shape[0], upscale, min_size, fix_resize)
    return u8_to_nchw_f32(resize_u8(u8, (w, h), plan), plan.lut("stage2", u8.device)), h0, w0


def caption_views(u8, processor, grid_pinpoints, dtype=_torch.float16, plan=None):
    """``llava_next.process_anyres_image`` of a device HWC uint8 RGB image -> ``dtype`` [1 + tiles, 3, S, S] on its device, equal bit for
    bit to the host function's result ``.to(dtype)``: Pillow's resize to the fitted size and to S x S (``resize_u8``; a pass that
    changes no size is skipped), then ``clip_views``.  Five launches at most, on the current stream; with the tables of ``plan``
    warm the host neither waits for the device nor copies from it."""
    from . import llava_next as LN
    fn = "caption_views"
    _image_u8(fn, "u8", u8)
    O._arg(fn, "u8", u8, _torch.uint8, shape=(None, None, 3))
    if dtype not in _VIEW_DT:
        raise L.RsvldOperandError(f"{fn}: dtype must be one of {tuple(_VIEW_DT)}, got {dtype!r}")
    if not u8.is_cuda:
        O._bad(fn, "u8", "must live on the GPU (the views are made where the image is; the host route is llava_next.process_images)")
    plan = ImagePlan() if plan is None else plan
    S = LN._proc_sizes(processor)[0]
    layout = anyres_layout((u8.shape[1], u8.shape[0]), S, grid_pinpoints)
    lut = plan.clip_lut(processor, dtype, u8.device)
    fit = resize_u8(u8, layout[2:4], plan) if tuple(layout[2:4]) != (u8.shape[1], u8.shape[0]) else u8
    whole = resize_u8(u8, (S, S), plan) if (S, S) != (u8.shape[1], u8.shape[0]) else u8
    return clip_views(whole, fit, lut, layout, dtype)


def tensor2pil_u8(x, h0, w0, plan=None):
    """``models.util.Tensor2PIL`` of an fp32 [3, H, W] device tensor -> device uint8 [h0, w0, 3] (``Image.fromarray`` of its host copy
    is the PIL image).  At equal sizes torch's bicubic is the identity, and the quantiser runs alone."""
    _image_f32("tensor2pil_u8", "x", x)
    plan = ImagePlan() if plan is None else plan
    h0, w0 = int(h0), int(w0)
    if (h0, w0) == tuple(x.shape[1:]):
        return nchw_f32_to_u8(x, MODE_TENSOR2PIL)
    return bicubic_f32_to_u8(x, plan.aten(x.shape[1], h0, x.device), plan.aten(x.shape[2], w0, x.device))
