"""``PipelineConfig.device_io`` in the caption stage of the driver (infer.py): the views come from the device uint8 image --
Stage 1's own copy of its hand-off image, or an upload -- through ``llava_next.process_images_device`` instead of PIL on the host, and
the caption is the same string.  The pipeline stub of tests/test_gpu_infer.py::test_live_llava_caption_on_device (tiny seeded
LLaVA-NeXT, seed 3); on the device route ``llava_next.process_images`` is replaced by a function that raises, so the host route is
provably not taken."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

SIZES = [(100, 70), (60, 150), (56, 56)]      # three different grids: 2 x 2, 1 x 3, 1 x 2


@pytest.fixture(scope="module")
def stub(cuda, tmp_path_factory):
    """-> (pipeline stub, the three images, their captions on the host route one by one, and as one batch)."""
    import llava_common as C
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel
    from rsvld_amd import infer, llava_next as LN
    tmp = tmp_path_factory.mktemp("caption_views")
    tower_dir = C.save_tiny_clip(str(tmp / "clip"))
    cfg = LN._llama_config_cls()(**C.LLAMA, **C.MM, mm_vision_tower=tower_dir)
    cfg._attn_implementation = "sdpa"
    model = LN.build_model(cfg, clip=CLIPVisionModel(CLIPVisionConfig(**C.VISION))).eval()
    C.name_seeded_state(model, C.WEIGHT_SEED)
    model.to(device=cuda, dtype=torch.float16)
    pipe = infer.SuperResolutionPipeline.__new__(infer.SuperResolutionPipeline)      # only the caption stage is under test
    pipe.cfg = infer.PipelineConfig(input_img=str(tmp / "x.png"), output_dir=str(tmp / "out"), seed=3, base_model_device="cuda:0")
    pipe.llava_model, pipe.llava_tokenizer = model, C.build_tokenizer()
    pipe.llava_image_processor = CLIPImageProcessor.from_pretrained(tower_dir)
    images = [C.test_image(size, 5 + n) for n, size in enumerate(SIZES)]
    assert not pipe.cfg.device_io
    host = [pipe.run_stage2_captioning(im) for im in images]
    host_batch = pipe.run_stage2_captioning_batch(images)
    assert all(isinstance(t, str) and t for t in host) and host_batch == host
    return pipe, images, host


@pytest.fixture
def device_route(stub, monkeypatch):
    """The stub with ``device_io`` on and the host's view function booby-trapped; both undone afterwards."""
    from rsvld_amd import llava_next as LN
    pipe = stub[0]

    def trap(*a, **k):
        raise AssertionError("device_io: the caption stage took the host route (llava_next.process_images)")

    monkeypatch.setattr(LN, "process_images", trap)
    monkeypatch.setattr(pipe.cfg, "device_io", True)
    monkeypatch.setattr(pipe, "_handoff", None, raising=False)
    monkeypatch.setattr(pipe, "_image_plan", None, raising=False)
    return pipe


def _u8(cuda, img):
    return torch.from_numpy(np.array(img, dtype=np.uint8)).to(cuda)


def test_the_trap_works(stub, device_route):
    """With ``device_io`` off the stage calls ``process_images`` -- the function the other tests replace."""
    device_route.cfg.device_io = False
    with pytest.raises(AssertionError, match="host route"):
        device_route.run_stage2_captioning(stub[1][0])


def test_caption_from_the_held_handoff_image(cuda, stub, device_route):
    _, images, host = stub
    # the device copy alone decides the views: the PIL image held beside it is a blank of the same size
    from PIL import Image
    blank = Image.new("RGB", images[0].size)
    device_route._handoff = (blank, _u8(cuda, images[0]))
    assert device_route.run_stage2_captioning(blank) == host[0]
    assert device_route._image_plan is not None and any(k[0] == "clip" for k in device_route._image_plan._tables)


def test_caption_from_an_uploaded_image(cuda, stub, device_route):
    _, images, host = stub
    assert device_route.run_stage2_captioning(images[1]) == host[1]                 # nothing held
    device_route._handoff = (images[0], _u8(cuda, images[0]))
    assert device_route.run_stage2_captioning(images[2]) == host[2]                 # another image is held


def test_a_grey_image_raises(stub, device_route):
    from rsvld_amd import _lib as L
    with pytest.raises(L.RsvldError, match="RGB"):
        device_route.run_stage2_captioning(stub[1][0].convert("L"))
    with pytest.raises(L.RsvldError, match="RGB"):
        device_route.run_stage2_captioning_batch([stub[1][0], stub[1][1].convert("L")])


def test_caption_batch_on_three_grids(cuda, stub, device_route):
    _, images, host = stub
    device_route._handoff = (images[1], _u8(cuda, images[1]))                       # the middle one is held, the others go up
    assert device_route.run_stage2_captioning_batch(images) == host
