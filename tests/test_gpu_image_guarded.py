"""Every wrapper of rsvld_amd/imageops.py on poisoned, guard-banded buffers (tests/guarded.py): operands and tables between guard
bands, outputs and intermediates through the arena, the result bit-identical to the plain call.

The poison byte 0xFF is a legal uint8 value, so the operands are chosen such that no correct uint8 output holds it, and
``_no_poison`` is the element test of the uint8 results: a byte left unwritten shows as 0xFF.
* images inside [64, 160]: the filters' absolute weights sum to less than 1.6 over both passes, so no output leaves [35, 189];
* tensors inside [-0.9, 0.9] quantise to at most 242;
* tensors inside [-0.4, 0.4] for the fp32 bicubic (absolute weights 1.375 per axis): it stays below 0.76, i.e. below 225.
fp32 results use the default test (0xFF.. is NaN)."""
import numpy as np
import pytest
import torch
from PIL import Image

import guarded

pytestmark = pytest.mark.gpu


def _no_poison(name, t):
    return (t != guarded.POISON) if t.dtype == torch.uint8 else None


def _image(cuda, w, h, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(64, 161, (h, w, 3), dtype=np.uint8)).to(cuda)


def _tensor(cuda, h, w, seed=0, amp=0.9):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-amp, amp, (3, h, w)).astype(np.float32)).to(cuda)


def _dev(cuda, arrays):
    return tuple(torch.from_numpy(a).to(cuda) for a in arrays)


@pytest.mark.parametrize("axis,size,out,first,out_len", [(0, (37, 21), 100, 0, None), (0, (37, 21), 100, 13, 64), (0, (130, 9), 64, 0, None),
                                                         (1, (37, 21), 50, 0, None), (1, (48, 21), 50, 7, 33), (1, (64, 70), 32, 0, None)])
def test_resample_u8_guarded(cuda, axis, size, out, first, out_len):
    """Both axes, the byte and the 16-byte vertical kernels (row pitches 111 and 144 / 192 bytes), a first-output offset, ksize 5 / 11."""
    from rsvld_amd import imageops as I
    src = _image(cuda, *size)
    table = _dev(cuda, I.pillow_bicubic_table(size[axis], out))
    got, _ = guarded.run_guarded(lambda src, table: I.resample_u8(src, table, axis, first, out_len), {"src": src, "table": table},
                                 expect=f"resample_u8_{'hv'[axis]}", finite=_no_poison)
    want = I.apply_pillow_table(src.cpu().numpy(), I.pillow_bicubic_table(size[axis], out), axis, first, out_len)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("W", [33, 64])
def test_converters_guarded(cuda, W):
    from rsvld_amd import imageops as I
    lut = torch.from_numpy(I.stage2_lut()).to(cuda)
    guarded.run_guarded(I.u8_to_nchw_f32, {"src": _image(cuda, W, 19), "lut": lut}, expect="u8_hwc_to_nchw_f32")
    for mode in (I.MODE_TENSOR2IMG, I.MODE_TENSOR2PIL):
        guarded.run_guarded(lambda x: I.nchw_f32_to_u8(x, mode), {"x": _tensor(cuda, 19, W)}, expect="nchw_f32_to_u8_hwc", finite=_no_poison)
    guarded.run_guarded(I.tensor2img, {"tensor": _tensor(cuda, 19, W).unsqueeze(0)}, expect="nchw_f32_to_u8_hwc", finite=_no_poison)


@pytest.mark.parametrize("size,out", [((19, 33), (23, 37)), ((40, 64), (31, 50)), ((8, 8), (64, 64))])
def test_bicubic_guarded(cuda, size, out):
    """Up, down, and x8 on a tiny image (every tap index clamped at some output)."""
    from rsvld_amd import imageops as I
    x = _tensor(cuda, *size, amp=0.4)
    ty, tx = _dev(cuda, I.aten_bicubic_table(size[0], out[0])), _dev(cuda, I.aten_bicubic_table(size[1], out[1]))
    got, _ = guarded.run_guarded(I.bicubic_f32_to_u8, {"x": x, "table_y": ty, "table_x": tx}, expect="bicubic_f32_to_u8_hwc", finite=_no_poison)
    assert np.array_equal(got.cpu().numpy(), I.bicubic_quantise_numpy(x.cpu().numpy(), *out))


def test_mirrors_of_the_host_functions_guarded(cuda):
    """resize_u8 (both passes, one pass, the copy, a crop window), pil2tensor, tensor2pil_u8 and load_sr_input: their intermediates
    come from the arena too.  The plan's tables are ordinary device tensors here (test_resample_u8_guarded guards tables)."""
    from rsvld_amd import imageops as I
    plan = I.ImagePlan()
    src = _image(cuda, 45, 31)
    for size, box in [((128, 64), None), ((45, 64), None), ((90, 31), None), ((45, 31), None), ((90, 64), (13, 0, 64, 64)), ((45, 62), (3, 5, 40, 40))]:
        got, _ = guarded.run_guarded(lambda src: I.resize_u8(src, size, plan, box), {"src": src}, finite=_no_poison)
        assert np.array_equal(got.cpu().numpy(), I.pillow_resize_numpy(src.cpu().numpy(), size, box))
    x, _ = guarded.run_guarded(lambda u8: I.pil2tensor(u8, 3, 64, 100, plan)[0], {"u8": src}, expect=("resample_u8_h", "resample_u8_v", "u8_hwc_to_nchw_f32"))
    assert tuple(x.shape) == (3, 128, 128) and I.pil2tensor(src, 3, 64, 100, plan)[1:] == (100, 145)
    guarded.run_guarded(lambda x: I.tensor2pil_u8(x, 100, 145, plan), {"x": _tensor(cuda, 128, 128, amp=0.4)}, expect="bicubic_f32_to_u8_hwc", finite=_no_poison)
    guarded.run_guarded(lambda x: I.tensor2pil_u8(x, 128, 128, plan), {"x": _tensor(cuda, 128, 128)}, expect="nchw_f32_to_u8_hwc", finite=_no_poison)
    img = Image.fromarray(src.cpu().numpy())
    sr, _ = guarded.run_guarded(lambda: I.load_sr_input(img, 2, cuda, plan)["SR"], {}, expect=("resample_u8_h", "resample_u8_v", "u8_hwc_to_nchw_f32"))
    assert tuple(sr.shape) == (1, 3, 90, 90)
