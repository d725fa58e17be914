"""``imageops.clip_views`` and ``imageops.caption_views`` on poisoned, guard-banded buffers (tests/guarded.py), in the manner of
tests/test_gpu_image_guarded.py: operands and the table between guard bands, the output and the two resized intermediates through the
arena, the result bit-identical to the plain call -- and the same again on a gated side stream, which ``run_guarded`` adds for device
operands.  The views are 16-bit or fp32 floats, so the default element test applies: an element left unwritten reads as NaN.

S = 17 and S = 30 (34- and 60-byte fp16 rows: no output row starts on a 16-byte boundary) with odd paste offsets."""
import numpy as np
import pytest
import torch
from PIL import Image

import caption_views_cases as CV
import guarded

pytestmark = pytest.mark.gpu

# S, canvas in tiles (gx, gy), fitted size (nw, nh), paste offset (ox, oy): free-hand rectangles, odd everywhere, one that touches the
# canvas's far corner and one of a single pixel
RECTS = [(17, (2, 2), (15, 21), (7, 5)), (17, (1, 2), (17, 11), (0, 11)), (17, (2, 1), (1, 1), (33, 16)),
         (30, (2, 2), (41, 33), (9, 13)), (30, (3, 1), (89, 29), (1, 1)), (30, (1, 3), (7, 77), (23, 13))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("S,grid,fit_size,offset", RECTS)
def test_clip_views_guarded(cuda, S, grid, fit_size, offset, dtype):
    from rsvld_amd import imageops as I
    (gx, gy), (nw, nh), (ox, oy) = grid, fit_size, offset
    rng = np.random.default_rng(S * nw + nh)
    whole, fit = rng.integers(0, 256, (S, S, 3), dtype=np.uint8), rng.integers(0, 256, (nh, nw, 3), dtype=np.uint8)
    lut = I.clip_lut(CV.processor(S), dtype)
    layout = (gx * S, gy * S, nw, nh, ox, oy)
    got, _ = guarded.run_guarded(lambda whole, fit, lut: I.clip_views(whole, fit, lut, layout, dtype),
                                 {"whole": torch.from_numpy(whole).to(cuda), "fit": torch.from_numpy(fit).to(cuda), "lut": lut.to(cuda)},
                                 expect="clip_views_u8")
    want = torch.from_numpy(I.assemble_views_numpy(whole, fit, lut.float().numpy(), layout)).to(dtype)
    assert tuple(got.shape) == (1 + gx * gy, 3, S, S) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("S,size,layout", [(17, (23, 40), (34, 34, 20, 34, 7, 0)), (17, (5, 3), (17, 34, 17, 11, 0, 11)),
                                           (30, (120, 98), (60, 60, 60, 49, 0, 5)), (30, (200, 9), (90, 30, 90, 5, 0, 12))])
def test_caption_views_guarded(cuda, S, size, layout):
    """The whole device route: the passes of both resizes and the views kernel, every intermediate in the arena.  The plan's tables are
    ordinary device tensors, warm after the plain call (``test_clip_views_guarded`` guards a table)."""
    from rsvld_amd import imageops as I, llava_next as LN
    assert I.anyres_layout(size, S, CV.PINS[S]) == layout
    plan, img = I.ImagePlan(), CV.image(size)
    got, rec = guarded.run_guarded(lambda u8: I.caption_views(u8, CV.processor(S), CV.PINS[S], torch.float16, plan),
                                   {"u8": torch.from_numpy(img).to(cuda)}, expect=("resample_u8_h", "resample_u8_v", "clip_views_u8"))
    assert rec.names[-1] == "clip_views_u8" and len(rec.names) == 5
    assert torch.equal(got.cpu(), LN.process_anyres_image(Image.fromarray(img), CV.processor(S), CV.PINS[S]).to(torch.float16))
