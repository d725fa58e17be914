"""The shapes of the caption-view tests (a helper module: nothing here is collected): CLIP image processors built in code, seeded
images, and ``CASES`` -- rows of (S, grid pinpoints, image (width, height)), the smallest shapes at which the assembly of the anyres
views can go wrong.  Shared by tests/test_caption_views_cases.py (CPU) and the three tests/test_gpu_caption_views*.py / _infer_ files."""
import functools

import numpy as np

PINS = {
    56: [[56, 112], [112, 56], [112, 112], [168, 56], [56, 168]],
    28: [[28, 56], [56, 28], [56, 56]],
    30: [[30, 60], [60, 30], [60, 60], [90, 30], [30, 90]],
    17: [[17, 34], [34, 17], [34, 34]],
    336: [[336, 672], [672, 336], [672, 672], [1008, 336], [336, 1008]],      # the 8 B model's (lmms-lab/llama3-llava-next-8b)
}

CASES = [
    (56, (100, 70)),      # pad above and below, 2 x 2 grid
    (56, (60, 150)),      # portrait, 1 x 3 grid
    (56, (56, 56)),       # one tile plus an empty tile
    (56, (640, 200)),     # nh = 53, oy = 1: an odd remainder
    (56, (57, 171)),      # exact fit, no padding
    (56, (31, 17)),       # up-scale
    (56, (1, 1)),
    (28, (37, 53)),       # pad LEFT and RIGHT, ox = 8
    (28, (56, 56)),       # canvas = image: both resizes skipped
    (30, (61, 47)),
    (30, (29, 88)),
    (30, (200, 9)),       # nh = 5
    (17, (23, 40)),       # ox = 7, odd row bytes
    (17, (5, 3)),
    (336, (700, 500)),
]
IDS = [f"S{S}-{w}x{h}" for S, (w, h) in CASES]
MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]


@functools.lru_cache(maxsize=None)
def processor(S, crop=None):
    """A CLIP image processor of edge ``S`` (crop ``S`` unless given), as tools/synthetic_models.py builds the 8 B model's."""
    from transformers import CLIPImageProcessor
    crop = S if crop is None else crop
    return CLIPImageProcessor(do_resize=True, size={"shortest_edge": S}, resample=3, do_center_crop=True,
                              crop_size={"height": crop, "width": crop}, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                              image_mean=MEAN, image_std=STD, do_convert_rgb=True)


def image(size, seed=0):
    """Seeded uint8 HWC noise of ``size`` = (width, height), every byte value in play."""
    return np.random.default_rng(1000 * size[0] + size[1] + seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def host_views(i):
    """``process_anyres_image`` of case ``i`` -> fp32 torch [1 + tiles, 3, S, S]: the reference, computed once and never modified."""
    from PIL import Image
    from rsvld_amd import llava_next as LN
    S, size = CASES[i]
    return LN.process_anyres_image(Image.fromarray(image(size)), processor(S), PINS[S])
