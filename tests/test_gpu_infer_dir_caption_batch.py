"""``infer_dir --caption_batch N`` end to end on the GPU, in the miniature of test_pipeline_with_live_caption_end_to_end
(tests/test_gpu_infer.py): 32-pixel tiles, 2 + 2 steps, the tiny seeded LLaVA-NeXT as the live captioner.  A folder of three images of
different aspect ratios gives byte-identical PNGs with ``caption_batch=3`` and ``caption_batch=1`` on the same pipeline object.

The tiny captioner's head dimension is not 128, so its batch goes through the one-after-another route of ``generate_batch``: what this
test pins is the grouped order of the stages and the generator hand-over (Stage 2 of an image starts from the state its Stage 1
left; every caption row seeded as the single call).  The batched kernels and loop are pinned in tests/test_gpu_decode_rows.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import s2_common as S

pytestmark = pytest.mark.gpu


def test_caption_batch_writes_the_pngs_of_the_one_by_one_loop(cuda, tmp_path):
    from PIL import Image
    import llava_common as C
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel
    from rsvld_amd import infer, llava_next as LN
    from rsvld_amd.infer_dir import ImageBatchProcessor
    cfg = yaml.safe_load(open(S.YAML.replace("juggernautXL.yaml", "juggernautXL_cached.yaml")))
    for k in ("control_stage_config", "network_config"):
        cfg["model"]["params"][k]["params"].update(S.SMALL)
    c, uc = S.cond_dicts()
    torch.save(c, tmp_path / "c.pth")
    torch.save(uc, tmp_path / "uc.pth")
    cfg["model"]["params"]["conditioner_config"]["params"] = {"cond_pth": str(tmp_path / "c.pth"), "un_cond_pth": str(tmp_path / "uc.pth")}
    cfg["SR_CKPT"] = cfg["SR_CKPT_Q"] = None
    yaml.safe_dump(cfg, open(tmp_path / "model.yaml", "w"))
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a", (32, 32)), ("b", (24, 32)), ("c", (32, 20))):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(src / f"{name}.png")
    extra = dict(model_yaml=str(tmp_path / "model.yaml"), allow_random_init=True, min_size=128)
    pc = infer.PipelineConfig(input_img=str(src / "a.png"), output_dir=str(tmp_path / "warm"), no_llava=True, upscale_factor=2, edm_steps=2,
                              sr3_steps=2, seed=1, img_threshold=0.3, base_model_device="cuda:0", **extra)
    pipe = infer.SuperResolutionPipeline(pc)                 # no_llava=True: nothing is loaded from disk ...
    tower_dir = C.save_tiny_clip(str(tmp_path / "clip"))     # ... the tiny captioner is put where load_llava() puts the 8 B one
    lcfg = LN._llama_config_cls()(**C.LLAMA, **C.MM, mm_vision_tower=tower_dir)
    lcfg._attn_implementation = "sdpa"
    llava = LN.build_model(lcfg, clip=CLIPVisionModel(CLIPVisionConfig(**C.VISION))).eval()
    C.name_seeded_state(llava, C.WEIGHT_SEED)
    pipe.llava_model, pipe.llava_tokenizer = llava.to(device=cuda, dtype=torch.float16), C.build_tokenizer()
    pipe.llava_image_processor = CLIPImageProcessor.from_pretrained(tower_dir)
    captions = []
    orig = pipe.refinement_model.just_sampling

    def spy(x, p, *a, **k):
        captions.append(p[0])
        return orig(x, p, *a, **k)

    pipe.refinement_model.just_sampling = spy
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p_ in pipe.refinement_model.parameters():
            if p_.dim() >= 2 and float(p_.abs().max()) == 0.0:
                p_.copy_((torch.randn(p_.shape, generator=g) * 0.02).to(p_.device))

    def run(n):
        proc = ImageBatchProcessor(str(src), str(tmp_path / f"out{n}"), upscale=2, num_steps=2, seed=1, img_threshold=0.3, sr3_steps=2,
                                   device="cuda:0", caption_batch=n)
        proc.kw.update(extra)
        proc.pipe = pipe
        del captions[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            done, failed = proc.run()
        assert not failed and sorted(os.path.basename(str(d)) for d in done) == ["a_final_0.png", "b_final_0.png", "c_final_0.png"]
        return list(captions)

    cap1, cap3 = run(1), run(3)
    assert len(cap1) == 3 and all(isinstance(t, str) and t for t in cap1) and cap3 == cap1      # live captions, the same in both orders
    for name in ("a", "b", "c"):
        for f in (f"sr3_{name}.png", f"{name}_final_0.png"):
            one, three = (tmp_path / "out1" / f).read_bytes(), (tmp_path / "out3" / f).read_bytes()
            assert one == three, f"{f}: caption_batch=3 wrote other bytes than caption_batch=1"
        assert np.asarray(Image.open(tmp_path / "out3" / f"{name}_final_0.png")).std() > 1.0
