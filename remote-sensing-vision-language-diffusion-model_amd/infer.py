"""Pipeline driver with the reference's CLI (infer.py:218-240) and stage order (:206-215):
Stage 1 SR3 upscale -> uint8 hand-off -> [caption] -> Stage 2 refinement -> PNG.

    python -m rsvld_amd.infer --input_img in.png --output_dir results --upscale_factor 8 --seed 42 \
        --img_threshold 0.3 --edm_steps 50 [--no_llava] [--caption "..."] [--sr3_steps 50]

Both diffusion stages run on ONE MI355X through librsvld_hip.so.  The LLaVA-Next captioner stays on stock
PyTorch-ROCm (rsvld_amd.llava_next: SDPA attention, seeded sampling); ``--no_llava`` skips it like the reference's
``no_llava`` and ``--caption`` supplies the text directly.  Its checkpoints must already be on disk
(``--llava_path`` / ``--llava_adapter``): nothing is fetched from the network."""
import argparse
from dataclasses import dataclass
from pathlib import Path

import torch
from PIL import Image

from . import imageops
from .configs import sr3 as SR3
from .data import dataset as SR_Dataset
from .llava_next import add_caption_arguments, caption_mode
from .models.util import PIL2Tensor, Tensor2PIL, create_SR_model
from .sr3_model import create_model
from .utils import logger as Logger
from .utils import tensor2img as T2I

_HERE = Path(__file__).resolve().parent


@dataclass
class PipelineConfig:
    """Field-for-field the reference's PipelineConfig (infer.py:21-69) minus the LLaVA device."""
    input_img: str
    output_dir: str = "./results"
    model_yaml: str = str(_HERE / "model_configs" / "juggernautXL.yaml")
    sr_model_device: str = "cuda:0"
    upscale_factor: int = 8
    a_prompt: str = ("Cinematic, High Contrast, highly detailed aerial photo taken using a high-resolution drone or satellite, "
                     "hyper detailed photo-realistic maximum detail, 32k, Color Grading, ultra HD, "
                     "extreme meticulous detailing of terrain textures and structures, hyper sharpness, no deformations.")
    n_prompt: str = ("painting, oil painting, illustration, drawing, art, sketch, oil painting, cartoon, CG Style, "
                     "3D render, unreal engine, blurring, dirty, messy, worst quality, low quality, frames, watermark, "
                     "signature, jpeg artifacts, deformed, lowres, over-smooth, cloud cover, heavy fog, motion blur, lens flare")
    min_size: int = 1024
    edm_steps: int = 50
    s_churn: int = 5
    s_noise: float = 1.003
    s_cfg: float = 7.5
    s_stage1: int = -1
    s_stage2: float = 1.0
    img_threshold: float = 0.3
    seed: int = -1
    num_samples: int = 1
    color_fix_type: str = "Wavelet"
    linear_cfg: bool = True
    linear_s_stage2: bool = False
    spt_linear_cfg: float = 4.0
    spt_linear_s_stage2: float = 0.0
    ae_dtype: str = "bf16"            # applied to the loaded Stage-2 model (the reference carries the two fields but never reads
    diff_dtype: str = "fp16"          # them); "fp32" = the fp32-operand kernel family: the reference's CPU result to ~1e-5
    sr3_dtype: str = "fp16"           # own field: Stage-1 UNet compute type; "fp32" = the reference's own Stage-1 precision; "w2" = fp16 tensors x weight pairs
    no_llava: bool = False
    caption: str = ""                 # when non-empty it is used as the caption and LLaVA is not loaded
    prompt_yaml: str = str(_HERE / "prompts" / "prompt_config.yaml")
    base_model_device: str = "cuda:0" # the reference puts LLaVA on a second GPU (cuda:1); one MI355X holds everything
    llava_path: str = "lmms-lab/llama3-llava-next-8b"
    llava_adapter: str = "./CKPT_PTH/Llava-next"
    use_tile_vae: bool = False
    encoder_tile_size: int = 512
    decoder_tile_size: int = 64
    sr3_steps: int = 0            # 0 = the option file's 'val' schedule (500 steps, configs/sr_sr3.json)
    allow_random_init: bool = False   # tests / benchmarks only: run without checkpoints on seeded random weights
    overlap_vae_with_caption: bool = True   # Stage 2's opening VAE passes on a second HIP stream beside the live caption pass
    device_io: bool = False           # resize / crop / 8-bit conversions around both stages on the GPU (rsvld_amd.imageops) instead of PIL + numpy + CPU torch
    caption_weights: str = "native"   # weights of the caption pass's token loop: "native" = the checkpoint's 16-bit ones, "e4m3" = e4m3 bytes + a scale per row (opt-in, rsvld_amd.w8), "e4m3-only" = the prefill on them too and the 16-bit decoder weights released (llava_next.CAPTION_WEIGHTS)
    caption_prefill: str = "torch"    # attention of the caption pass's prefill: "torch" = the stock-torch sequence over the whole cache, "flash" = the causal flash kernel (opt-in, rsvld_amd.prefill_attention)
    caption_decode: str = "valu"      # kernels of the token loop's products: "valu" = the vector-ALU ones, "mfma" = on MFMAs, whose arithmetic does not grow with --caption_batch (opt-in, csrc/gemv_mma.hip; llava_next.CAPTION_DECODES)
    caption_attention: str = "valu"   # attention of the token loop: "valu" = da_kernel on the vector ALU, "mfma" = key tiles by LDS-DMA, scores and P V on MFMAs (opt-in, dam_kernel of csrc/decode_attention.hip; llava_next.CAPTION_ATTENTIONS)

    def __post_init__(self):
        caption_mode(self.caption_weights, self.caption_prefill, self.caption_decode, self.caption_attention, who="PipelineConfig",
                     names=("caption_weights", "caption_prefill", "caption_decode", "caption_attention"))
        self.output_dir = Path(self.output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.input_path = Path(self.input_img)
        self.filename = self.input_path.stem


class SuperResolutionPipeline:
    _side_stream = None     # ONE second HIP stream for every image's VAE front (the caching allocator keys its free blocks by stream)
    _image_plan = None      # device_io: the device tables of rsvld_amd.imageops, built on first use and kept for every image
    _handoff = None         # device_io: (the PIL hand-off image of the current input, the device uint8 it is the host copy of)

    def __init__(self, cfg: PipelineConfig):
        self.cfg = cfg
        if cfg.seed >= 0:
            torch.manual_seed(cfg.seed)
        self.llava_model = self.llava_tokenizer = self.llava_image_processor = None
        self._load_sr3_model()
        if not cfg.no_llava and not cfg.caption:
            self._load_llava_model()
        self._load_refinement_model()

    def _load_sr3_model(self):
        opt = Logger.parse(SR3.SR3_Config(), allow_random_init=self.cfg.allow_random_init)
        self.sr3_model = create_model(opt)
        self.sr3_model.netG.denoise_fn.set_compute_dtype(self.cfg.sr3_dtype)
        sched = dict(opt["model"]["beta_schedule"]["val"])
        if self.cfg.sr3_steps > 0:
            sched["n_timestep"] = self.cfg.sr3_steps
        self.sr3_model.set_new_noise_schedule(sched, schedule_phase="val")

    def _load_llava_model(self):
        from .models.util import load_llava
        self.llava_tokenizer, self.llava_model, self.llava_image_processor = load_llava(
            device=self.cfg.base_model_device, model_path=self.cfg.llava_path, adapter_path=self.cfg.llava_adapter)

    def _load_refinement_model(self):
        self.refinement_model = create_SR_model(self.cfg.model_yaml, allow_random_init=self.cfg.allow_random_init)
        if self.refinement_model is None:
            raise RuntimeError(f"{self.cfg.model_yaml}: SR_CKPT is null, there are no pretrained weights to refine with")
        self.refinement_model.to(self.cfg.sr_model_device)
        self.refinement_model.set_precision(self.cfg.ae_dtype, self.cfg.diff_dtype)
        if self.cfg.use_tile_vae:
            self.refinement_model.init_tile_vae(self.cfg.encoder_tile_size, self.cfg.decoder_tile_size)

    def _plan(self):
        if self._image_plan is None:
            self._image_plan = imageops.ImagePlan()
        return self._image_plan

    def run_stage1_sr3_upscale(self, image_path: Path) -> Image.Image:
        if self.cfg.device_io:
            # the decoded LR image goes up as uint8; resize, centre crop and the [-1, 1] conversion are kernels
            val_data = imageops.load_sr_input(str(image_path), self.cfg.upscale_factor, self.sr3_model.device, self._plan())
        else:
            val_data = SR_Dataset.load_sr_input(str(image_path), self.cfg.upscale_factor)
        self.sr3_model.feed_data(val_data)
        self.sr3_model.test(continous=True)
        sr = self.sr3_model.SR
        if sr.dim() == 4:
            sr = sr[-1]
        if self.cfg.device_io:
            # quantised on the device: the uint8 image comes down (a quarter of the fp32 tensor) for the PNG and the caption pass,
            # and stays up for Stage 2
            u8 = imageops.tensor2img(sr, min_max=(-1, 1))
            sr_pil = Image.fromarray(u8.cpu().numpy())
            self._handoff = (sr_pil, u8)
        else:
            sr_pil = Image.fromarray(T2I.tensor2img(sr, min_max=(-1, 1)))      # 8-bit hand-off, as the reference
        sr_pil.save(self.cfg.output_dir / f"sr3_{self.cfg.filename}.png")
        return sr_pil

    def _caption_views(self, sr_image):
        """The views the captioner sees of one Stage-1 image: a one-element list of fp16 [1 + tiles, 3, S, S] on ``base_model_device``."""
        from . import llava_next as LN
        dev = self.cfg.base_model_device
        if self.cfg.device_io:
            # resized, tiled and normalised where the image already is (Stage 1's device copy of its hand-off image; any other image
            # is uploaded as uint8), on the current stream -- the stream ``tensor2img`` wrote it on and the caption runs on
            held = self._handoff is not None and self._handoff[0] is sr_image
            if not held and sr_image.mode != "RGB":
                raise imageops.L.RsvldError(f"device_io: the caption pass takes an RGB image, got mode {sr_image.mode!r}")
            u8 = self._handoff[1] if held else imageops.upload_u8(sr_image, dev)
            return list(LN.process_images_device([u8.to(dev)], self.llava_image_processor, self.llava_model.config, torch.float16,
                                                 self._plan()))
        views = LN.process_images([sr_image], self.llava_image_processor, self.llava_model.config)
        return [v.to(dtype=torch.float16, device=dev) for v in views]

    def run_stage2_captioning(self, sr_image) -> str:
        """infer.py:145-166: caption of the Stage-1 image.  Returns the caption STRING handed to just_sampling as p[0]
        (the reference passes get_img_describe's one-element list straight through as ``[caption]``; the text is the same)."""
        if self.cfg.caption:
            return self.cfg.caption
        if self.cfg.no_llava or self.llava_model is None:
            return ""
        import yaml
        from . import llava_next as LN
        with open(self.cfg.prompt_yaml, "r", encoding="utf-8") as f:
            img_prompt = yaml.safe_load(f)["img_prompt"].format(DEFAULT_IMAGE_TOKEN=LN.DEFAULT_IMAGE_TOKEN)
        dev = self.cfg.base_model_device
        views = self._caption_views(sr_image)
        # a fixed --seed makes the caption reproducible too (sampled inside a forked generator: Stage 2's noise draws do not
        # depend on how many tokens were sampled); --seed < 0 means "random run": the caption samples from the current state
        seed = None if self.cfg.seed < 0 else self.cfg.seed
        return LN.get_img_describe(image_tensor=views, image=sr_image, model=self.llava_model, tokenizer=self.llava_tokenizer,
                                   prompt=img_prompt, max_new_tokens=256, device=dev, seed=seed,
                                   decode_weights=self.cfg.caption_weights, decode_prefill=self.cfg.caption_prefill,
                                   decode_kernel=self.cfg.caption_decode, decode_attention=self.cfg.caption_attention)[0]

    def run_stage2_captioning_batch(self, sr_images):
        """``run_stage2_captioning`` for the Stage-1 images of several inputs in ONE token loop (``infer_dir --caption_batch``) -> a list
        of caption strings, each the string ``run_stage2_captioning`` returns for that image alone (every row is seeded as the single
        call seeds it; ``llava_next.FastDecoder.generate_batch``)."""
        if self.cfg.caption:
            return [self.cfg.caption] * len(sr_images)
        if self.cfg.no_llava or self.llava_model is None:
            return [""] * len(sr_images)
        import yaml
        from . import llava_next as LN
        with open(self.cfg.prompt_yaml, "r", encoding="utf-8") as f:
            img_prompt = yaml.safe_load(f)["img_prompt"].format(DEFAULT_IMAGE_TOKEN=LN.DEFAULT_IMAGE_TOKEN)
        dev = self.cfg.base_model_device
        views = [self._caption_views(im) for im in sr_images]
        seeds = None if self.cfg.seed < 0 else [self.cfg.seed] * len(sr_images)
        return LN.get_img_describe_batch(image_tensors=views, images=list(sr_images), model=self.llava_model, tokenizer=self.llava_tokenizer,
                                         prompt=img_prompt, max_new_tokens=256, device=dev, seeds=seeds,
                                         decode_weights=self.cfg.caption_weights, decode_prefill=self.cfg.caption_prefill,
                                         decode_kernel=self.cfg.caption_decode, decode_attention=self.cfg.caption_attention)

    def _stage2_input(self, sr_image):
        if self.cfg.device_io:
            # Stage 1's own device copy when ``sr_image`` is its hand-off image; any other image is uploaded as uint8
            held = self._handoff is not None and self._handoff[0] is sr_image
            if not held and sr_image.mode != "RGB":      # (Pillow resizes an image with alpha through premultiplied alpha: no kernel for that)
                raise imageops.L.RsvldError(f"device_io: Stage 2 takes an RGB image, got mode {sr_image.mode!r}")
            u8 = self._handoff[1] if held else imageops.upload_u8(sr_image, self.cfg.sr_model_device)
            lq, h0, w0 = imageops.pil2tensor(u8.to(self.cfg.sr_model_device), upscale=1, min_size=self.cfg.min_size, plan=self._plan())
            return lq.unsqueeze(0)[:, :3], h0, w0
        lq, h0, w0 = PIL2Tensor(sr_image, upscale=1, min_size=self.cfg.min_size)
        return lq.unsqueeze(0).to(self.cfg.sr_model_device)[:, :3], h0, w0

    def start_vae_front(self, sr_image):
        """Issue the three VAE passes that open Stage 2 (they depend on the image only) on a second HIP stream, so that they run BESIDE
        the caption pass -- a weight-streaming token loop that leaves the matrix pipes idle -- instead of after it.  -> a handle for
        ``run_stage3_refinement(..., front=...)``; same kernels and the same random draws as the serial order."""
        lq, h0, w0 = self._stage2_input(sr_image)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=lq.device)
        side = self._side_stream
        side.wait_stream(torch.cuda.current_stream(lq.device))
        with torch.cuda.stream(side):
            front = self.refinement_model.vae_front(lq, self.cfg.num_samples, restoration_scale=self.cfg.s_stage1)
        return side, front, (lq, h0, w0)

    def run_stage3_refinement(self, sr_image, caption: str, front=None):
        if front is None:
            lq, h0, w0 = self._stage2_input(sr_image)
            vae_front = None
        else:
            side, vae_front, (lq, h0, w0) = front
            torch.cuda.current_stream(lq.device).wait_stream(side)
            for t in vae_front:
                if t is not None:      # (z_stage1 is None while the restoration pull is off)
                    t.record_stream(torch.cuda.current_stream(lq.device))
        c = self.cfg
        samples = self.refinement_model.just_sampling(
            lq, [caption], num_steps=c.edm_steps, restoration_scale=c.s_stage1, s_churn=c.s_churn, s_noise=c.s_noise,
            cfg_scale=c.s_cfg, control_scale=c.s_stage2, seed=c.seed, num_samples=c.num_samples, p_p=c.a_prompt,
            n_p=c.n_prompt, color_fix_type=c.color_fix_type, use_linear_CFG=c.linear_cfg,
            use_linear_control_scale=c.linear_s_stage2, cfg_scale_start=c.spt_linear_cfg,
            control_scale_start=c.spt_linear_s_stage2, img_threshold=c.img_threshold, dec_img=1, vae_front=vae_front)
        outs = []
        for i, s in enumerate(samples):
            path = c.output_dir / f"{c.filename}_final_{i}.png"
            if c.device_io:      # bicubic back to the hand-off size and the 8-bit quantiser in one kernel; only the uint8 image comes down
                Image.fromarray(imageops.tensor2pil_u8(s.float().contiguous(), h0, w0, plan=self._plan()).cpu().numpy()).save(path)
            else:
                Tensor2PIL(s, h0, w0).save(path)
            outs.append(path)
        return outs

    def process(self):
        sr3 = self.run_stage1_sr3_upscale(self.cfg.input_path)
        live = not (self.cfg.caption or self.cfg.no_llava or self.llava_model is None)
        front = self.start_vae_front(sr3) if (live and self.cfg.overlap_vae_with_caption) else None
        return self.run_stage3_refinement(sr3, self.run_stage2_captioning(sr3), front=front)


def build_parser():
    p = argparse.ArgumentParser(description="MI355X-native two-stage super-resolution pipeline")
    p.add_argument("--input_img", type=str, required=True)
    p.add_argument("--output_dir", type=str, default="./results")
    p.add_argument("--upscale_factor", type=int, default=8)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--img_threshold", type=float, default=0.3)
    p.add_argument("--edm_steps", type=int, default=50)
    p.add_argument("--sr3_steps", type=int, default=0)
    p.add_argument("--caption", type=str, default="")
    p.add_argument("--no_llava", action="store_true")
    p.add_argument("--llava_path", type=str, default="lmms-lab/llama3-llava-next-8b")
    p.add_argument("--llava_adapter", type=str, default="./CKPT_PTH/Llava-next")
    p.add_argument("--use_tile_vae", action="store_true")
    p.add_argument("--device_io", action="store_true", help="resize, crop and the 8-bit conversions around both stages on the GPU "
                   "(rsvld_amd.imageops; bit-identical to the host route except one 8-bit step in a few bytes per 100 000 of a resized final image)")
    p.add_argument("--fp32", action="store_true", help="both stages on the fp32-operand kernels (reference CPU-path precision; slow)")
    p.add_argument("--tolerance", action="store_true", help="the tolerance-compliant composition (what bench.py times): inside 1e-3 of the reference's CPU path after 50 + 50 steps at ~1.3 x "
                   "the default's time.  Stage 1: fp16 tensors x fp16 weight pairs (two MFMAs per product); Stage 2: fp32 residual "
                   "streams, convolutions as three bf16 MFMAs on hi + lo operands, attention operands and the to_out / FeedForward / "
                   "q|k|v inputs in fp16 x weight pairs (rsvld_amd.ops.UNET_POLICY), the VAE all three-MFMA")
    p.add_argument("--split", action="store_true", help="both stages in the split-operand mode: fp32 tensors, matrix products as three 16-bit "
                                                         "MFMAs on hi + lo bf16 operands (~1e-5 per product) -- except the layer inputs the "
                                                         "default policy hands over in fp16 (attention operands, to_out / FeedForward / q|k|v "
                                                         "inputs: rsvld_amd.ops.UNET_POLICY; fp16 x weight pairs, two MFMAs)")
    p.add_argument("--vae_split", action="store_true", help="only the VAE passes in the split-operand mode (the shipped fp16 UNets): "
                                                             "+3 %% time, Stage-2 distance from the CPU path 3e-3 instead of 3e-2")
    add_caption_arguments(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    cfg = PipelineConfig(input_img=a.input_img, output_dir=a.output_dir, upscale_factor=a.upscale_factor, seed=a.seed,
                         img_threshold=a.img_threshold, edm_steps=a.edm_steps, sr3_steps=a.sr3_steps, caption=a.caption,
                         no_llava=a.no_llava, llava_path=a.llava_path, llava_adapter=a.llava_adapter, use_tile_vae=a.use_tile_vae,
                         device_io=a.device_io, caption_weights=a.caption_weights, caption_prefill=a.caption_prefill,
                         caption_decode=a.caption_decode, caption_attention=a.caption_attention,
                         **(dict(ae_dtype="fp32", diff_dtype="fp32", sr3_dtype="fp32") if a.fp32 else
                            dict(ae_dtype="split", diff_dtype="split", sr3_dtype="w2") if a.tolerance else
                            dict(ae_dtype="split", diff_dtype="split", sr3_dtype="split") if a.split else
                            dict(ae_dtype="split") if a.vae_split else {}))
    SuperResolutionPipeline(cfg).process()


if __name__ == "__main__":
    main()
