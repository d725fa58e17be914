"""``imageops.caption_views`` -- the caption's anyres views made on the device from a resident uint8 image -- against the host route
``llava_next.process_anyres_image(...).to(dtype)`` on every row of tests/caption_views_cases.py: ``torch.equal``, no tolerance
(the resizes are Pillow's integer arithmetic from host-built tables, the normalisation is a table read off the processor)."""
import pytest
import torch

import caption_views_cases as CV

pytestmark = pytest.mark.gpu

BF16_ROWS = (3, 12)      # S56-640x200 (odd remainder) and S17-23x40 (odd offset, 34-byte rows)


def _device_views(cuda, i, dtype, plan=None):
    from rsvld_amd import imageops as I
    S, size = CV.CASES[i]
    u8 = torch.from_numpy(CV.image(size)).to(cuda)
    return I.caption_views(u8, CV.processor(S), CV.PINS[S], dtype, plan), u8


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("i", range(len(CV.CASES)), ids=CV.IDS)
def test_caption_views_equal_the_host_route(cuda, i, dtype):
    got, u8 = _device_views(cuda, i, dtype)
    want = CV.host_views(i).to(dtype)
    assert got.device == u8.device and got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("i", BF16_ROWS, ids=[CV.IDS[i] for i in BF16_ROWS])
def test_caption_views_bf16(cuda, i):
    got, _ = _device_views(cuda, i, torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), CV.host_views(i).to(torch.bfloat16))


def _names(fn):
    from rsvld_amd import ops
    with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
        fn()
    return [r[0] for r in prof.records]


def test_launches_and_tables(cuda):
    """Five launches where both resizes change both sizes, fewer where a pass changes none, the views kernel alone where the canvas is
    the image; a second call through the same plan builds no table."""
    from PIL import Image
    from rsvld_amd import imageops as I, llava_next as LN
    H, V, K = "resample_u8_h", "resample_u8_v", "clip_views_u8"
    plan = I.ImagePlan()
    for i, want in ((0, [H, V, H, V, K]),       # (100, 70): fit 112 x 79, then the squash to 56 x 56
                    (8, [H, V, K]),             # (56, 56), S = 28: the canvas is the image, only the squash runs
                    (2, [K])):                  # (56, 56), S = 56: the image is its own fit and its own squash
        assert _names(lambda: _device_views(cuda, i, torch.float16, plan)) == want, CV.IDS[i]
        n = len(plan._tables)
        again, _ = _device_views(cuda, i, torch.float16, plan)
        assert len(plan._tables) == n and torch.equal(again.cpu(), CV.host_views(i).to(torch.float16))
    assert sum(k[0] == "clip" for k in plan._tables) == 2         # one table per processor setting (S = 56, S = 28), not per image
    # (56, 100), S = 56: the image is its own fit; the squash changes the height only
    img = CV.image((56, 100))
    assert I.anyres_layout((56, 100), 56, CV.PINS[56]) == (56, 112, 56, 100, 0, 6)
    got = []
    names = _names(lambda: got.append(I.caption_views(torch.from_numpy(img).to(cuda), CV.processor(56), CV.PINS[56], torch.float16, plan)))
    assert names == [V, K]
    assert torch.equal(got[0].cpu(), LN.process_anyres_image(Image.fromarray(img), CV.processor(56), CV.PINS[56]).to(torch.float16))


def test_operand_contracts(cuda):
    from rsvld_amd import _lib as L, imageops as I
    proc, pins = CV.processor(56), CV.PINS[56]
    img = torch.from_numpy(CV.image((100, 70)))
    with pytest.raises(L.RsvldOperandError, match="dtype"):
        I.caption_views(img.to(cuda).float(), proc, pins)
    with pytest.raises(L.RsvldOperandError, match="shape"):
        I.caption_views(torch.cat([img, img[..., :1]], dim=2).to(cuda), proc, pins)
    with pytest.raises(L.RsvldOperandError, match="GPU"):
        I.caption_views(img, proc, pins)
    with pytest.raises(L.RsvldOperandError, match="dtype"):
        I.caption_views(img.to(cuda), proc, pins, dtype=torch.float64)
    # clip_views: the table's type, the fitted image's shape and a rectangle that leaves the canvas
    whole, fit = torch.zeros((56, 56, 3), dtype=torch.uint8, device=cuda), torch.zeros((79, 112, 3), dtype=torch.uint8, device=cuda)
    lut = I.clip_lut(proc, torch.float16).to(cuda)
    layout = I.anyres_layout((100, 70), 56, pins)
    assert layout == (112, 112, 112, 79, 0, 16)
    assert tuple(I.clip_views(whole, fit, lut, layout).shape) == (5, 3, 56, 56)
    for bad in (dict(lut=lut.float()), dict(fit=fit[:78]), dict(layout=(112, 112, 112, 79, 0, 34)), dict(layout=(112, 100, 112, 79, 0, 16)),
                dict(whole=whole[:, :55]), dict(layout=(112, 112, 112, 79, 1, 16))):
        args = dict(whole=whole, fit=fit, lut=lut, layout=layout)
        args.update(bad)
        with pytest.raises(L.RsvldOperandError):
            I.clip_views(**args)


def test_entry_point_refuses_bad_arguments(cuda):
    """The host side of the C entry point itself: a rectangle outside the canvas and an unknown dtype come back as error codes."""
    from rsvld_amd import _lib as L, ops as O
    lib = L.load()
    whole, fit = torch.zeros((17, 17, 3), dtype=torch.uint8, device=cuda), torch.zeros((5, 9, 3), dtype=torch.uint8, device=cuda)
    lut, dst = torch.zeros((3, 256), dtype=torch.float16, device=cuda), torch.zeros((3, 3, 17, 17), dtype=torch.float16, device=cuda)

    def call(S=17, nw=9, nh=5, ox=7, oy=6, gx=2, gy=1, dtype=L.F16):
        return lib.rsvld_clip_views_u8(O._ptr(whole), O._ptr(fit), O._ptr(lut), O._ptr(dst), S, nw, nh, ox, oy, gx, gy, dtype, O._stream())

    assert call() == 0
    assert call(ox=26) == call(oy=13) == call(nw=0) == call(ox=-1) == call(gy=0) == -1
    assert call(dtype=L.SPLIT) == call(dtype=7) == -2
    torch.cuda.synchronize()
