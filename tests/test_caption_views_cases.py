"""The host side of the caption views on the device (rsvld_amd/imageops.py), on the CPU: the numpy restatement of
``llava_next.process_anyres_image`` equals it bit for bit on every row of tests/caption_views_cases.py, the layout helper equals what a
pasted white image shows, the measured CLIP table equals ``preprocess`` and refuses processors that are no per-byte table -- and the
comparison itself bites: five faults built into the restatement are each rejected by at least one row."""
import numpy as np
import pytest
import torch
from PIL import Image

import caption_views_cases as CV


@pytest.mark.parametrize("i", range(len(CV.CASES)), ids=CV.IDS)
def test_restatement_equals_process_anyres_image(i):
    from rsvld_amd import imageops as I
    S, size = CV.CASES[i]
    want = CV.host_views(i)
    got = I.caption_views_numpy(CV.image(size), CV.processor(S), CV.PINS[S])
    assert want.dtype == torch.float32 and got.dtype == np.float32 and got.shape == tuple(want.shape)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))
    # and after the rounding of the product's route (fp16): the 16-bit table is the fp32 table rounded
    lut16 = I.clip_lut(CV.processor(S), torch.float16)
    assert torch.equal(lut16, I.clip_lut(CV.processor(S)).to(torch.float16)) and lut16.dtype == torch.float16


@pytest.mark.parametrize("i", range(len(CV.CASES)), ids=CV.IDS)
def test_anyres_layout_equals_a_pasted_white_image(i):
    """The canvas size, and the bounding box of what is not black after ``resize_and_pad_image`` of a white image."""
    from rsvld_amd import imageops as I, llava_next as LN
    S, size = CV.CASES[i]
    tw, th, nw, nh, ox, oy = I.anyres_layout(size, S, CV.PINS[S])
    canvas = LN.resize_and_pad_image(Image.new("RGB", size, (255, 255, 255)),
                                     LN.select_best_resolution(size, LN._resolutions(CV.PINS[S], S)))
    assert canvas.size == (tw, th) and tw % S == 0 and th % S == 0
    assert (tw // S, th // S) == LN.anyres_grid_shape(size, CV.PINS[S], S)
    lit = np.asarray(canvas).max(axis=2) > 0
    ys, xs = np.nonzero(lit.any(axis=1))[0], np.nonzero(lit.any(axis=0))[0]
    assert (xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1) == (ox, oy, nw, nh)
    assert lit[oy:oy + nh, ox:ox + nw].all()


@pytest.mark.parametrize("S", [17, 30, 56])
def test_clip_lut_equals_preprocess(S):
    from rsvld_amd import imageops as I
    proc = CV.processor(S)
    lut = I.clip_lut(proc)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and not lut.is_cuda
    img = CV.image((S, S), seed=7)
    want = proc.preprocess(Image.fromarray(img), return_tensors="pt")["pixel_values"][0]
    got = torch.stack([lut[c][torch.from_numpy(img[..., c].astype(np.int64))] for c in range(3)])
    assert torch.equal(got, want)
    assert float(lut[0, 0]) != 0.0 and len({float(lut[c, 0]) for c in range(3)}) == 3      # normalised black: not 0, and per channel
    plan = I.ImagePlan()
    a = plan.clip_lut(proc, torch.float32, "cpu")
    assert plan.clip_lut(CV.processor(S), torch.float32, "cpu") is a and torch.equal(a, lut) and len(plan._tables) == 1


class _Flipping:
    """A stand-in whose ``preprocess`` mirrors the image first: pointwise arithmetic, but not at the same pixel."""

    def __init__(self, proc):
        self._p, self.size, self.crop_size = proc, proc.size, proc.crop_size
        self.image_mean, self.image_std = proc.image_mean, proc.image_std

    def preprocess(self, img, **kw):
        return self._p.preprocess(img.transpose(Image.FLIP_LEFT_RIGHT), **kw)


def test_clip_lut_refuses_what_is_no_table():
    from rsvld_amd import _lib as L, imageops as I
    with pytest.raises(L.RsvldError, match="crops"):
        I.clip_lut(CV.processor(56, crop=48))
    with pytest.raises(L.RsvldError, match="one byte, two values"):
        I.clip_lut(_Flipping(CV.processor(56)))
    with pytest.raises(L.RsvldError, match="one byte, two values"):
        I.clip_lut(_Flipping(CV.processor(16)))            # one pixel per byte: only the shuffled probe can tell
    with pytest.raises(L.RsvldError, match="256 byte values"):
        I.clip_lut(CV.processor(15))
    assert tuple(I.clip_lut(CV.processor(16)).shape) == (3, 256)


# ---------------------------------------------------------------------------------------- the comparison bites
def _restate(u8, S, fault):
    """``imageops.caption_views_numpy`` with one fault built in (None: none)."""
    from rsvld_amd import imageops as I
    proc, pins = CV.processor(S), CV.PINS[S]
    lut = I.clip_lut(proc).numpy()
    tw, th, nw, nh, ox, oy = I.anyres_layout((u8.shape[1], u8.shape[0]), S, pins)
    fit, whole = I.pillow_resize_numpy(u8, (nw, nh)), I.pillow_resize_numpy(u8, (S, S))
    if fault == "offset":
        ox, oy = (tw - nw + 1) // 2, (th - nh + 1) // 2
    if fault == "channels":
        lut = lut[::-1]
    if fault == "view0":                       # view 0 cut from the canvas instead of the squashed image
        canvas = np.zeros((th, tw, 3), np.uint8)
        canvas[oy:oy + nh, ox:ox + nw] = fit
        whole = canvas[:S, :S]
    out = I.assemble_views_numpy(whole, fit, lut, (tw, th, nw, nh, ox, oy))
    if fault == "zero_pad":                    # padding written as 0.0 instead of the table's value of byte 0
        mask = np.zeros((th, tw), bool)
        mask[oy:oy + nh, ox:ox + nw] = True
        for v in range(1, out.shape[0]):
            ty, tx = divmod(v - 1, tw // S)
            out[v][:, ~mask[ty * S:(ty + 1) * S, tx * S:(tx + 1) * S]] = 0.0
    if fault == "column_major":
        gx, gy = tw // S, th // S
        order = [1 + ty * gx + tx for tx in range(gx) for ty in range(gy)]
        out = np.concatenate([out[:1], out[order]], axis=0)
    return out


def test_the_unfaulted_variant_is_the_restatement():
    from rsvld_amd import imageops as I
    for i, (S, size) in enumerate(CV.CASES[:9]):
        assert np.array_equal(_restate(CV.image(size), S, None), I.caption_views_numpy(CV.image(size), CV.processor(S), CV.PINS[S]))


@pytest.mark.parametrize("fault", ["zero_pad", "offset", "column_major", "view0", "channels"])
def test_each_fault_is_rejected_by_some_row(fault):
    rejected = [CV.IDS[i] for i, (S, size) in enumerate(CV.CASES)
                if not np.array_equal(_restate(CV.image(size), S, fault), CV.host_views(i).numpy())]
    print(f"{fault}: rejected by {rejected}")
    assert rejected
