"""``PipelineConfig.device_io``: the whole driver (infer.py) with the image steps on the GPU against the same pipeline object with them
on the host -- reduced network depth (the setup of tests/test_gpu_infer.py::test_pipeline_cli_flow), default precision, 3 + 3 steps,
``torch.manual_seed`` before each run.  Everything up to Stage 2's input is bit-identical; the final image too unless it is resized
back (``Tensor2PIL``'s fp32 bicubic: one 8-bit step in at most 0.1 % of the bytes; the restatement of tests/test_image_tables.py
predicts fewer than one byte of the 12 288)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import s2_common as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(cuda, tmp_path_factory):
    from PIL import Image
    from rsvld_amd import infer
    tmp = tmp_path_factory.mktemp("device_io")
    cfg = yaml.safe_load(open(S.YAML.replace("juggernautXL.yaml", "juggernautXL_cached.yaml")))
    for k in ("control_stage_config", "network_config"):
        cfg["model"]["params"][k]["params"].update(S.SMALL)
    c, uc = S.cond_dicts()
    torch.save(c, tmp / "c.pth")
    torch.save(uc, tmp / "uc.pth")
    cfg["model"]["params"]["conditioner_config"]["params"] = {"cond_pth": str(tmp / "c.pth"), "un_cond_pth": str(tmp / "uc.pth")}
    cfg["SR_CKPT"] = cfg["SR_CKPT_Q"] = None
    yaml.safe_dump(cfg, open(tmp / "model.yaml", "w"))
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(tmp / "square.png")
    Image.fromarray(rng.integers(0, 255, (24, 32, 3), dtype=np.uint8)).save(tmp / "tile.png")
    p = infer.SuperResolutionPipeline(_config(tmp, "square", False))
    # zero-initialised output convs would make Stage 2 a no-op: give them small seeded weights
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p_ in p.refinement_model.parameters():
            if p_.dim() >= 2 and float(p_.abs().max()) == 0.0:
                p_.copy_((torch.randn(p_.shape, generator=g) * 0.02).to(p_.device))
    return p, tmp


def _config(tmp, name, device_io):
    from rsvld_amd import infer
    return infer.PipelineConfig(input_img=str(tmp / f"{name}.png"), output_dir=str(tmp / f"out_{name}_{'dev' if device_io else 'host'}"),
                                model_yaml=str(tmp / "model.yaml"), allow_random_init=True, no_llava=True, upscale_factor=2,
                                min_size=128, edm_steps=3, sr3_steps=3, seed=1, img_threshold=0.3, device_io=device_io)


def _both_routes(pipe, name):
    """-> {device_io: (sr3 image, the tensor Stage 2 was given, final image)} of one ``process()`` per route."""
    from PIL import Image
    p, tmp = pipe
    orig, res = p.refinement_model.just_sampling, {}
    for device_io in (False, True):
        p.cfg = _config(tmp, name, device_io)
        seen = {}

        def spy(x, *a, **k):
            seen["lq"] = x.detach().clone()
            return orig(x, *a, **k)

        p.refinement_model.just_sampling = spy
        try:
            torch.manual_seed(1)
            outs = p.process()
        finally:
            p.refinement_model.just_sampling = orig
        assert [os.path.basename(o) for o in outs] == [f"{name}_final_0.png"]
        sr3 = Image.open(p.cfg.output_dir / f"sr3_{name}.png")
        lq, h0, w0 = p._stage2_input(sr3)                    # from the PNG: the upload path of the device route
        assert seen["lq"].is_cuda and torch.equal(lq, seen["lq"])
        res[device_io] = (np.asarray(sr3), seen["lq"].cpu(), (h0, w0), np.asarray(Image.open(outs[0])))
    return res


def test_device_io_no_size_changes(pipe):
    """LR 64 x 64, x2, min_size 128: 128 -> 128 -> 128, neither resizer of Stage 2 runs; every file is identical."""
    r = _both_routes(pipe, "square")
    assert r[True][0].shape == (128, 128, 3) and np.array_equal(r[True][0], r[False][0])
    assert r[True][1].shape == (1, 3, 128, 128) and torch.equal(r[True][1], r[False][1]) and r[True][2] == r[False][2] == (128, 128)
    assert r[True][3].shape == (128, 128, 3) and r[False][3].std() > 1.0 and np.array_equal(r[True][3], r[False][3])


def test_device_io_both_resizers(pipe):
    """LR 24 x 32: 64 -> 128 -> 64: the loader crops, PIL2Tensor upsamples, Tensor2PIL resizes back."""
    r = _both_routes(pipe, "tile")
    assert r[True][0].shape == (64, 64, 3) and np.array_equal(r[True][0], r[False][0])
    assert r[True][1].shape == (1, 3, 128, 128) and torch.equal(r[True][1], r[False][1]) and r[True][2] == r[False][2] == (64, 64)
    d = np.abs(r[True][3].astype(np.int64) - r[False][3].astype(np.int64))
    print(f"final image, device route vs host route: max step {d.max()}, {int((d > 0).sum())} of {d.size} bytes differ")
    assert d.size == 12288 and r[False][3].std() > 1.0
    assert d.max() <= 1 and (d > 0).sum() <= 0.001 * d.size
