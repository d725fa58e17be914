"""Model factory + image <-> tensor helpers (reference: models/util.py:73-108,132-166)."""
import os

import numpy as np
import torch
import yaml

from ..sgm.util import AttrDict, instantiate_from_config


def get_state_dict(d):
    return d.get("state_dict", d)


def load_state_dict(ckpt_path, location="cpu"):
    _, ext = os.path.splitext(ckpt_path)
    if ext.lower() == ".safetensors":
        import safetensors.torch
        sd = safetensors.torch.load_file(ckpt_path, device=location)
    else:
        sd = get_state_dict(torch.load(ckpt_path, map_location=torch.device(location)))
    return get_state_dict(sd)


def load_config(path):
    with open(path, "r", encoding="utf-8") as f:
        return AttrDict(yaml.safe_load(f))


def create_SR_model(config_path, load_default_setting=False, allow_random_init=False):
    """yaml -> SR_backbone, then the two checkpoints (SDXL base, SR adapter) with strict=False, in the order of
    models/util.py:93-108.  Like the reference, ``SR_CKPT: null`` means "no pretrained weights" and returns None --
    unless ``allow_random_init`` (tests, benchmarks) asks for the randomly initialised model.  A CONFIGURED checkpoint
    path that does not exist raises FileNotFoundError (the reference fails inside torch.load): nothing is skipped
    silently."""
    import logging
    log = logging.getLogger("rsvld_amd")
    config = load_config(config_path)
    model = instantiate_from_config(config.model).cpu()
    if config.get("SR_CKPT") is None:
        if not allow_random_init:
            print("There are no pretrained weights.")
            return None
        log.warning("create_SR_model: SR_CKPT is null, returning a RANDOMLY INITIALISED model (allow_random_init=True)")
    else:
        for key in ("SR_CKPT", "SR_CKPT_Q"):
            path = config.get(key)
            if path is None or not os.path.exists(path):
                raise FileNotFoundError(f"create_SR_model: {key} = {path!r} (from {config_path}) does not exist")
            res = model.load_state_dict(load_state_dict(path), strict=False)
            log.info("create_SR_model: loaded %s (%d missing, %d unexpected keys)", path, len(res.missing_keys),
                     len(res.unexpected_keys))
            if res.unexpected_keys:
                log.warning("create_SR_model: unexpected keys in %s, e.g. %s", path, res.unexpected_keys[:5])
    if load_default_setting:
        return model, config.default_setting
    return model


def load_llava(device="cuda", **kw):
    """(tokenizer, model, image_processor) of the LLaVA-NeXT captioner (models/util.py:111-117), loaded ROCm-clean
    (SDPA attention, no flash-attn / bitsandbytes; see rsvld_amd.llava_next)."""
    from ..llava_next import load_llava as _load
    return _load(device=device, **kw)


def get_img_describe(*args, **kw):
    """models/util.py:17-66 (same signature, plus ``seed``)."""
    from ..llava_next import get_img_describe as _describe
    return _describe(*args, **kw)


def pil2tensor_size(w, h, upscale=1, min_size=1024, fix_resize=None):
    """-> (w, h, h0, w0): the x64 size ``PIL2Tensor`` resizes a (w, h) image to and the hand-off size it reports (the device route,
    rsvld_amd.imageops.pil2tensor, takes its sizes from here too)."""
    w *= upscale
    h *= upscale
    w0, h0 = round(w), round(h)
    if min(w, h) < min_size:
        s = min_size / min(w, h)
        w *= s
        h *= s
    if fix_resize is not None:
        s = fix_resize / min(w, h)
        w *= s
        h *= s
        w0, h0 = round(w), round(h)
    w = int(np.round(w / 64.0)) * 64
    h = int(np.round(h / 64.0)) * 64
    return w, h, h0, w0


def PIL2Tensor(img, upscale=1, min_size=1024, fix_resize=None):
    """PIL.Image -> Tensor[C,H,W] RGB in [-1,1]; sides rounded to multiples of 64 (util.py:132-156)."""
    from PIL import Image
    w, h, h0, w0 = pil2tensor_size(*img.size, upscale, min_size, fix_resize)
    x = img.resize((w, h), Image.BICUBIC)
    x = np.array(x).round().clip(0, 255).astype(np.uint8)
    x = x / 255 * 2 - 1
    return torch.tensor(x, dtype=torch.float32).permute(2, 0, 1), h0, w0


def Tensor2PIL(x, h0, w0):
    """Tensor[C,H,W] RGB in [-1,1] -> PIL.Image of size (w0, h0) (util.py:159-166)."""
    from PIL import Image
    x = torch.nn.functional.interpolate(x.unsqueeze(0).float().cpu(), size=(h0, w0), mode="bicubic")
    x = (x.squeeze(0).permute(1, 2, 0) * 127.5 + 127.5).numpy().clip(0, 255).astype(np.uint8)
    return Image.fromarray(x)


def convert_dtype(dtype_str):
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype_str]
