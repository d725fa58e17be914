"""The device image path (csrc/image.hip through rsvld_amd/imageops.py) against the yardsticks of the host route: the reference's
own outputs in tests/golden/host_prepost.npz and stage1_loader.npz (the arrays tests/test_host_prepost.py pins the host functions
to), Pillow itself, and the host functions on the quantisers' edge values.  Bit for bit everywhere except ``Tensor2PIL``'s fp32
bicubic, which is within one 8-bit step in at most 2e-4 of the bytes (tests/test_image_tables.py has the reasoning)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_STEP, MAX_FRACTION = 1, 2e-4


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE if name.startswith("test_") else os.path.join(HERE, "golden"),
                                                                     name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


CASES = _module("test_host_prepost").CASES
LOADER_CASES = _module("gen_loader_golden").CASES


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "host_prepost.npz"))


@pytest.fixture(scope="module")
def plan():
    from rsvld_amd import imageops as I
    return I.ImagePlan()


def _noisy(gold, i):
    x = torch.tensor(gold[f"p2t{i}_u8"] / 255 * 2 - 1, dtype=torch.float32)
    return (x + torch.from_numpy(gold[f"noise{i}"]).float()).clamp(-1.2, 1.2)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_pil2tensor_and_tensor2img_equal_the_reference_outputs(cuda, gold, plan, i):
    from rsvld_amd import imageops as I
    (w, h), up, ms, fr = CASES[i]
    u8 = torch.from_numpy(gold[f"in{i}"]).to(cuda)
    assert tuple(u8.shape) == (h, w, 3)
    x, h0, w0 = I.pil2tensor(u8, upscale=up, min_size=ms, fix_resize=fr, plan=plan)
    want = torch.tensor(gold[f"p2t{i}_u8"] / 255 * 2 - 1, dtype=torch.float32)
    assert x.is_cuda and x.dtype == torch.float32 and torch.equal(x.cpu(), want)
    assert [h0, w0] == list(gold[f"p2t{i}_hw"])
    got = I.tensor2img(_noisy(gold, i).unsqueeze(0).to(cuda))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), gold[f"t2i{i}"])


def test_tensor2pil_within_the_cap_of_the_reference_outputs(cuda, gold, plan):
    """Pooled over the five cases; beside the cap, the kernel equals its numpy restatement (same fp32 operations in the same order,
    nothing contracted) bit for bit."""
    from rsvld_amd import imageops as I
    differ = total = 0
    for i in range(len(CASES)):
        y = _noisy(gold, i)
        h0, w0 = (int(v) for v in gold[f"p2t{i}_hw"])
        got = I.tensor2pil_u8(y.to(cuda), h0, w0, plan=plan)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (h0, w0, 3)
        got = got.cpu().numpy()
        d = np.abs(got.astype(np.int64) - gold[f"t2p{i}"].astype(np.int64))
        print(f"case {i}: {tuple(y.shape[1:])} -> {(h0, w0)}: max step {d.max()}, {int((d > 0).sum())} of {d.size} bytes differ")
        assert d.max() <= MAX_STEP
        differ, total = differ + int((d > 0).sum()), total + d.size
        restated = I.bicubic_quantise_numpy(y.numpy(), h0, w0) if (h0, w0) != tuple(y.shape[1:]) else \
            I.quantise_numpy(y.numpy(), I.MODE_TENSOR2PIL).transpose(1, 2, 0)
        assert np.array_equal(got, restated)
    print(f"pooled: {differ} of {total} bytes differ ({differ / total:.2e})")
    assert differ <= MAX_FRACTION * total


def test_load_sr_input_equals_the_loader_fixture(cuda, plan, tmp_path):
    """stage1_loader.npz, and three more geometries against the host loader itself: w < h, w > h with an odd crop offset."""
    from rsvld_amd import imageops as I
    from rsvld_amd.data.dataset import load_sr_input, resize_geometry
    z = np.load(os.path.join(HERE, "golden", "stage1_loader.npz"))
    for i, ((w, h), s) in enumerate(LOADER_CASES):
        img = Image.fromarray(z[f"in{i}"])
        want = ((z[f"out{i}_u8"].astype(np.float32) / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)
        got = I.load_sr_input(img, s, cuda, plan=plan)
        side = int(max(w, h) * s)
        assert got["SR"].is_cuda and tuple(got["SR"].shape) == (1, 3, side, side) and int(got["Index"][0]) == 0
        assert torch.equal(got["SR"].cpu(), torch.from_numpy(want)), (i, w, h, s)
    rng = np.random.default_rng(11)
    for (w, h), s in [((21, 32), 4), ((32, 20), 4), ((32, 21), 3)]:
        img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        p = str(tmp_path / f"lr_{w}_{h}.png")
        img.save(p)
        got = I.load_sr_input(p, s, cuda, plan=plan)["SR"]                 # from a path, like the host loader
        assert torch.equal(got.cpu(), load_sr_input(p, s)["SR"]), (w, h, s, resize_geometry(w, h, s))
    assert any(resize_geometry(w, h, s)[3] % 2 or resize_geometry(w, h, s)[4] % 2 for (w, h), s in [((32, 21), 3), ((21, 32), 4)])


def _edge_values():
    f = np.float32
    k = np.arange(255, dtype=np.float64)
    ties = ((2 * k + 1) / 255 - 1).astype(f)                  # tensor2img: u * 255 = k + 0.5
    cuts = (np.arange(256, dtype=np.float64) / 127.5 - 1).astype(f)   # Tensor2PIL: x * 127.5 + 127.5 = k
    vals = [f([0.0, 1.0, -1.0, 1.2, -1.2])]
    for v in (ties, cuts):
        vals += [v, np.nextafter(v, f(-2)), np.nextafter(v, f(2))]
    return np.concatenate(vals)


def test_quantiser_edge_values_equal_the_host_functions(cuda):
    """0.0 (127.5 -> 128), +-1, +-1.2, the fp32 values nearest the rounding ties (2k+1)/255 - 1 and the truncation boundaries
    k/127.5 - 1, each with its fp32 neighbour on either side: a product contracted into an FMA, or a rounding mode, shows here."""
    from rsvld_amd import imageops as I
    from rsvld_amd.models.util import Tensor2PIL
    from rsvld_amd.utils.tensor2img import tensor2img
    v = _edge_values()
    W = 33
    H = -(-v.size // (3 * W))
    x = np.zeros(3 * H * W, np.float32)
    x[:v.size] = v
    x = torch.from_numpy(x.reshape(3, H, W))
    assert np.asarray(Tensor2PIL(torch.zeros(3, 2, 2), 2, 2))[0, 0, 0] == 127 and tensor2img(torch.zeros(3, 2, 2))[0, 0, 0] == 128
    assert np.array_equal(I.tensor2img(x.to(cuda)).cpu().numpy(), tensor2img(x.clone()))
    assert np.array_equal(I.tensor2pil_u8(x.to(cuda), H, W).cpu().numpy(), np.asarray(Tensor2PIL(x, H, W)))


@pytest.mark.parametrize("src,dst", [((33, 9), (37, 45)), ((37, 20), (45, 33)), ((45, 7), (33, 37)),      # odd widths: byte tails
                                     ((3, 5), (64, 64)),                                                  # n < ksize on both sides
                                     ((64, 64), (512, 512)),                                              # x8, 16-byte vertical pass
                                     ((130, 70), (64, 64)),                                               # ksize 11
                                     ((96, 64), (96, 128)), ((96, 64), (48, 64)), ((96, 64), (96, 64))])  # one pass skipped / a copy
def test_resize_u8_equals_pillow(cuda, plan, src, dst):
    from rsvld_amd import imageops as I
    a = np.random.default_rng(src[0] + dst[0]).integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    dev = torch.from_numpy(a).to(cuda)
    got = I.resize_u8(dev, dst, plan)
    assert got.data_ptr() != dev.data_ptr() and tuple(got.shape) == (dst[1], dst[0], 3)
    assert np.array_equal(got.cpu().numpy(), np.asarray(Image.fromarray(a).resize(dst, Image.BICUBIC)))


@pytest.mark.parametrize("W", [33, 37, 45])
def test_converters_on_odd_widths(cuda, plan, W):
    from rsvld_amd import imageops as I
    a = np.random.default_rng(W).integers(0, 256, (19, W, 3), dtype=np.uint8)
    for kind, lut in (("stage2", I.stage2_lut()), ("loader", I.loader_lut())):
        got = I.u8_to_nchw_f32(torch.from_numpy(a).to(cuda), plan.lut(kind, cuda))
        assert torch.equal(got.cpu(), torch.from_numpy(lut[a]).permute(2, 0, 1))
    x = torch.from_numpy(np.random.default_rng(W).uniform(-1.3, 1.3, (3, 19, W)).astype(np.float32))
    for mode in (I.MODE_TENSOR2IMG, I.MODE_TENSOR2PIL):
        assert np.array_equal(I.nchw_f32_to_u8(x.to(cuda), mode).cpu().numpy(), I.quantise_numpy(x.numpy(), mode).transpose(1, 2, 0))
    got = I.tensor2pil_u8(x.to(cuda), 23, W + 4, plan=plan).cpu().numpy()
    assert np.array_equal(got, I.bicubic_quantise_numpy(x.numpy(), 23, W + 4))


def test_other_ranges_are_refused(cuda):
    from rsvld_amd import _lib as L, imageops as I
    with pytest.raises(L.RsvldError):
        I.tensor2img(torch.zeros(3, 8, 8, device=cuda), min_max=(0, 1))
