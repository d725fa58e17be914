"""The host-built tables of the device image path (rsvld_amd/imageops.py), without a GPU: applied in numpy with the kernels'
arithmetic they reproduce Pillow's 8-bit bicubic resize and the two look-up tables bit for bit, and ``Tensor2PIL``'s fp32 bicubic
within one 8-bit step in at most 2e-4 of the bytes (a plain fp32 restatement in another summation order than ATen's differs from it
in 2e-5 to 4e-5 of the bytes on these shapes; the cap leaves 5x)."""
import numpy as np
import pytest
import torch
from PIL import Image

RESIZE_CASES = [((37, 53), (128, 192)), ((50, 40), (128, 128)), ((64, 64), (512, 512)), ((130, 70), (128, 64)),
                ((45, 31), (128, 64)), ((33, 33), (264, 264)), ((96, 64), (96, 64)),
                ((3, 5), (64, 64)),            # n < ksize on both sides of every output
                ((96, 64), (96, 128))]         # the vertical pass only
BICUBIC_CASES = [((192, 192), (177, 177)), ((128, 192), (100, 150)), ((64, 64), (96, 96))]
MAX_STEP, MAX_FRACTION = 1, 2e-4


def _image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_pillow_tables_reproduce_image_resize(src, dst):
    from rsvld_amd import imageops as I
    a = _image(*src, seed=src[0] * 1000 + dst[0])
    want = np.asarray(Image.fromarray(a).resize(dst, Image.BICUBIC))
    got = I.pillow_resize_numpy(a, dst)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_pillow_table_shape_and_bounds():
    from rsvld_amd import imageops as I
    for n_in, n_out in [(64, 512), (130, 64), (3, 64), (96, 96)]:
        bounds, coeffs = I.pillow_bicubic_table(n_in, n_out)
        ksize = 2 * int(np.ceil(2.0 * max(n_in / n_out, 1.0))) + 1
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
        assert bounds.shape == (n_out, 2) and coeffs.shape == (n_out, ksize)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert abs(int(coeffs.sum(1).max()) - (1 << 22)) <= ksize and abs(int(coeffs.sum(1).min()) - (1 << 22)) <= ksize
    b, c = I.identity_table(5)
    assert np.array_equal(I.apply_pillow_table(_image(5, 4, 1), (b, c), 0), _image(5, 4, 1))


def test_crop_window_equals_crop_of_the_resize():
    """``first`` / ``box``: the outputs a centre crop throws away are skipped, the kept ones do not change."""
    from rsvld_amd import imageops as I
    from rsvld_amd.data.dataset import resize_and_convert, resize_geometry
    for (w, h), s in [((21, 32), 4), ((32, 20), 4), ((16, 16), 2)]:
        a = _image(w, h, seed=w)
        nw, nh, target, left, top = resize_geometry(w, h, s)
        got = I.pillow_resize_numpy(a, (nw, nh), box=(left, top, target, target))
        assert np.array_equal(got, np.asarray(resize_and_convert(Image.fromarray(a), s)))


def test_lookup_tables_equal_the_host_expressions():
    from rsvld_amd import imageops as I
    v = np.arange(256).astype(np.uint8)
    stage2 = torch.tensor(v / 255 * 2 - 1, dtype=torch.float32).numpy()                  # models/util.py:PIL2Tensor
    loader = (((torch.from_numpy(v).float() / 255.0) - 0.5) / 0.5).numpy()             # data/dataset.py:load_sr_input
    assert I.stage2_lut().dtype == np.float32 and np.array_equal(I.stage2_lut(), stage2)
    assert I.loader_lut().dtype == np.float32 and np.array_equal(I.loader_lut(), loader)
    assert np.array_equal(stage2, np.float32(np.arange(256) / 255 * 2 - 1))


def test_quantisers_equal_the_host_functions():
    from rsvld_amd import imageops as I
    from rsvld_amd.models.util import Tensor2PIL
    from rsvld_amd.utils.tensor2img import tensor2img
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1.3, 1.3, (3, 40, 56)).astype(np.float32))
    assert np.array_equal(I.quantise_numpy(x.numpy(), I.MODE_TENSOR2IMG).transpose(1, 2, 0), tensor2img(x.clone()))
    assert np.array_equal(I.quantise_numpy(x.numpy(), I.MODE_TENSOR2PIL).transpose(1, 2, 0), np.asarray(Tensor2PIL(x, 40, 56)))


def test_aten_bicubic_tables_within_the_cap_of_tensor2pil():
    from rsvld_amd import imageops as I
    from rsvld_amd.models.util import Tensor2PIL
    differ = total = 0
    for k, ((h, w), (h0, w0)) in enumerate(BICUBIC_CASES):
        x = torch.from_numpy(np.random.default_rng(20 + k).uniform(-1.2, 1.2, (3, h, w)).astype(np.float32))
        want = np.asarray(Tensor2PIL(x, h0, w0)).astype(np.int64)
        got = I.bicubic_quantise_numpy(x.numpy(), h0, w0)
        assert got.dtype == np.uint8 and got.shape == (h0, w0, 3)
        d = np.abs(got.astype(np.int64) - want)
        print(f"bicubic {(h, w)} -> {(h0, w0)}: max step {d.max()}, {int((d > 0).sum())} of {d.size} bytes differ")
        assert d.max() <= MAX_STEP
        differ, total = differ + int((d > 0).sum()), total + d.size
    print(f"pooled: {differ} of {total} bytes differ ({differ / total:.2e})")
    assert differ <= MAX_FRACTION * total


def test_aten_bicubic_tables_are_the_identity_at_equal_size():
    from rsvld_amd import imageops as I
    from rsvld_amd.models.util import Tensor2PIL
    x = torch.from_numpy(np.random.default_rng(9).uniform(-1.2, 1.2, (3, 48, 80)).astype(np.float32))
    idx, w = I.aten_bicubic_table(48, 48)
    assert np.array_equal(idx[:, 1], np.arange(48)) and np.array_equal(w, np.tile(np.float32([0, 1, 0, 0]), (48, 1)))
    assert np.array_equal(I.bicubic_quantise_numpy(x.numpy(), 48, 80), np.asarray(Tensor2PIL(x, 48, 80)))


def test_wrappers_check_their_operands_before_the_gpu():
    """Contracts hold on CPU tensors (checked before the GPU-only check, as in ops.py), and there is no CPU path."""
    from rsvld_amd import _lib as L, imageops as I
    u8 = torch.zeros(8, 8, 3, dtype=torch.uint8)
    lut = torch.zeros(256)
    with pytest.raises(L.RsvldOperandError):
        I.u8_to_nchw_f32(u8.float(), lut)
    with pytest.raises(L.RsvldOperandError):
        I.u8_to_nchw_f32(u8, lut[:255])
    with pytest.raises(L.RsvldOperandError):
        I.nchw_f32_to_u8(torch.zeros(3, 8, 8, dtype=torch.float16), I.MODE_TENSOR2IMG)
    with pytest.raises(L.RsvldOperandError):
        I.nchw_f32_to_u8(torch.zeros(3, 8, 8).transpose(1, 2), I.MODE_TENSOR2PIL)
    tab = tuple(torch.from_numpy(a) for a in I.pillow_bicubic_table(8, 16))
    with pytest.raises(L.RsvldOperandError):
        I.resample_u8(u8, tab, 2)
    with pytest.raises(L.RsvldOperandError):
        I.resample_u8(u8, tab, 0, first=4, out_len=16)
    with pytest.raises(L.RsvldError):
        I.tensor2img(torch.zeros(3, 8, 8), min_max=(0, 1))
    with pytest.raises(L.RsvldError, match="GPU only"):
        I.u8_to_nchw_f32(u8, lut)
    with pytest.raises(L.RsvldError, match="GPU only"):
        I.tensor2pil_u8(torch.zeros(3, 8, 8), 8, 8)
