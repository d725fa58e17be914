"""LLaVA-NeXT caption pass on stock PyTorch-ROCm (BASELINE configs[3] "live LLaVA-Next prompt").

The reference runs a vendored LLaVA-NeXT tree (``llava/``, ~20 k lines) whose loader defaults to
``attn_implementation="flash_attention_2"`` (llava/model/builder.py:30) and wraps the model in a ``peft`` adapter
(models/util.py:111-117).  Per BASELINE.json north_star this pass stays a PyTorch module (it is conditioning, not the
hot path); what the build owns is a ROCm-clean way to load and drive it:

  * ``LlavaNextLlama``: transformers' own ``LlamaForCausalLM`` + ``CLIPVisionModel`` (SDPA attention -- no flash-attn, no
    bitsandbytes) with the multimodal members named as in the reference model (``model.vision_tower.vision_tower.*``,
    ``model.mm_projector.{0,2}``, ``model.image_newline``; llava/model/llava_arch.py:36-49), so the reference's
    ``lmms-lab/llama3-llava-next-8b`` checkpoint loads unchanged;
  * the "anyres" image path: tile selection, resize+pad, tiling (llava/mm_utils.py:121-296), CLIP layer -2 patch features
    -> 2-layer GELU MLP (multimodal_encoder/clip_encoder.py:48-82, multimodal_projector/builder.py:41-48), un-padding of
    the tile grid and one ``image_newline`` embedding per feature row (llava_arch.py:129-161,372-409), spliced into the
    token embeddings where the prompt holds IMAGE_TOKEN_INDEX (llava_arch.py:440-497);
  * ``get_img_describe`` with the reference's signature (models/util.py:17-66): Llama-3 chat template of
    ``conv_llava_llama_3`` (llava/conversation.py:98-110,387-398), sampling at temperature 0.2 -- plus an explicit
    ``seed`` so captions are reproducible;
  * ``merge_lora``: the adapter of ``./CKPT_PTH/Llava-next`` folded into the base weights (W += B A * alpha / r) when
    ``peft`` is not installed.

Pinned offline by tests/test_llava_next.py against token ids, input embeddings and logits the REFERENCE model produced on a
tiny seeded LLaMA + CLIP configuration (tests/golden/gen_llava_golden.py).
"""
import ast
import collections
import dataclasses
import json
import math
import os
import re
import time

import torch
from torch import nn

IGNORE_INDEX = -100
IMAGE_TOKEN_INDEX = -200            # llava/constants.py
DEFAULT_IMAGE_TOKEN = "<image>"
LLAMA3_SYSTEM = ("You are a helpful language and vision assistant. You are able to understand the visual content that the user "
                 "provides, and assist the user with a variety of tasks using natural language.")   # conversation.py:388
DEFAULT_MODEL = "lmms-lab/llama3-llava-next-8b"     # models/util.py:112-114
DEFAULT_ADAPTER = "./CKPT_PTH/Llava-next"           # models/util.py:115
# The caption pass's three user-level switches: PipelineConfig.caption_weights / caption_prefill / caption_decode, --caption_weights /
# --caption_prefill / --caption_decode of infer.py and infer_dir.py, decode_weights / decode_prefill / decode_kernel of
# get_img_describe(_batch), weights / prefill / decode of caption_tokens_fast(_batch).  ``caption_mode`` validates them -- it alone -- and
# maps them to the ``CaptionMode`` a ``FastDecoder`` is built and compared with.
# "e4m3-only": the prefill on the packs too and the 16-bit decoder weights released, CaptionMode(weights="e4m3", prefill_weights="e4m3",
# release_native=True).  Decodes: "valu" runs the weight-streaming products on the vector ALU (csrc/gemv.hip); "mfma" (opt-in) on MFMAs
# (csrc/gemv_mma.hip), whose arithmetic does not grow with the captions of a batch.  The two sum in different orders: other logits, the
# same contract each.  A fourth switch, caption_attention / --caption_attention / decode_attention / attention, picks the token loop's
# ATTENTION: "valu" is da_kernel of csrc/decode_attention.hip, "mfma" (opt-in) dam_kernel of the same unit -- key tiles by LDS-DMA, scores and P V
# on MFMAs, fp32 scores and a 16-bit P where "valu" has 16-bit scores and an fp32 P: other logits again, the same caches.
CAPTION_WEIGHTS = ("native", "e4m3", "e4m3-only")
CAPTION_PREFILLS = ("torch", "flash")
CAPTION_DECODES = ("valu", "mfma")
CAPTION_ATTENTIONS = ("valu", "mfma")


@dataclasses.dataclass(frozen=True)
class CaptionMode:
    """What a ``FastDecoder`` runs on, beyond its model and the size of its cache: the six switches its docstring describes.  The record
    owns every check of a value or a combination that needs no model; two decoders serve the same calls exactly when their records are
    equal (``_decoder_for``)."""
    weights: str = "native"
    prefill: str = "torch"
    prefill_weights: str = "native"
    release_native: bool = False
    decode: str = "valu"
    decode_attention: str = "valu"

    WEIGHTS = PREFILL_WEIGHTS = ("native", "e4m3")      # (un-annotated: class constants, not fields)

    def __post_init__(self):
        for name, allowed in (("decode", CAPTION_DECODES), ("weights", self.WEIGHTS), ("prefill", CAPTION_PREFILLS),
                              ("prefill_weights", self.PREFILL_WEIGHTS), ("decode_attention", CAPTION_ATTENTIONS)):
            if getattr(self, name) not in allowed:
                raise ValueError(f"FastDecoder: {name}={getattr(self, name)!r}, expected one of {allowed}")
        if self.prefill_weights == "e4m3" and self.weights != "e4m3":
            raise ValueError(f"FastDecoder: prefill_weights='e4m3' runs the prefill on the token loop's packs and requires weights='e4m3' "
                             f"(got weights={self.weights!r}; there is no fallback)")
        if self.release_native and self.prefill_weights != "e4m3":
            raise ValueError("FastDecoder: release_native=True requires prefill_weights='e4m3' (the 16-bit weights can only go once "
                             "nothing reads them)")


def caption_mode(weights=None, prefill=None, decode=None, attention=None, who="caption_mode", names=("weights", "prefill", "decode", "attention")):
    """The user-level values (a ``CAPTION_WEIGHTS``, a ``CAPTION_PREFILLS``, a ``CAPTION_DECODES`` and a ``CAPTION_ATTENTIONS`` value; None =
    the default, the first of its tuple) -> their ``CaptionMode``.  ``who`` / ``names``: the caller and what IT calls them, for the error
    (three names: the fourth is "attention")."""
    tuples = (CAPTION_WEIGHTS, CAPTION_PREFILLS, CAPTION_DECODES, CAPTION_ATTENTIONS)
    names = tuple(names) + ("attention",) * (len(tuples) - len(names))
    weights, prefill, decode, attention = (allowed[0] if v is None else v for v, allowed in zip((weights, prefill, decode, attention), tuples))
    for name, v, allowed in zip(names, (weights, prefill, decode, attention), tuples):
        if v not in allowed:
            raise ValueError(f"{who}: {name}={v!r}, expected one of {allowed}")
    only = weights == "e4m3-only"
    return CaptionMode(weights="e4m3" if only else weights, prefill=prefill, prefill_weights="e4m3" if only else "native", release_native=only,
                       decode=decode, decode_attention=attention)


def decoder_mode(caption_weights):
    """A ``CAPTION_WEIGHTS`` value -> the three weight fields of its ``CaptionMode``, as ``FastDecoder`` keywords."""
    mode = caption_mode(caption_weights, who="decoder_mode", names=("caption_weights", "prefill", "decode"))
    return dict(weights=mode.weights, prefill_weights=mode.prefill_weights, release_native=mode.release_native)


def add_caption_arguments(p, batch=False):
    """``--caption_weights``, ``--caption_prefill``, ``--caption_decode``, ``--caption_attention`` and (``batch``: the directory runner) ``--caption_batch`` on an
    argparse parser; the runner's help texts say what the option means for a group of captions."""
    p.add_argument("--caption_weights", choices=CAPTION_WEIGHTS, default="native", help="weights of the caption pass's token loop: " + (
        "the checkpoint's 16-bit ones, e4m3 bytes with a scale per row, or e4m3-only: the prefill on them too and the 16-bit "
        "decoder weights released (opt-in; see INTEGRATION.md)" if batch else
        "the checkpoint's 16-bit ones, or e4m3 bytes with one power-of-two scale per output row (half the bytes of a loop bound "
        "by nothing else; opt-in: fidelity on the real checkpoint is unmeasured; +8 GB beside the 16-bit weights); e4m3-only "
        "runs the prefill on those bytes too and releases the 16-bit decoder weights (one model throughout, 8 GB instead of 24)"))
    p.add_argument("--caption_prefill", choices=CAPTION_PREFILLS, default="torch", help="attention of the caption pass's prefill: the " + (
        "stock-torch sequence, or the library's causal flash kernel (opt-in; with it the captions of --caption_batch N no "
        "longer depend on the cache length a group was prefilled at; see DESIGN.md section 8)" if batch else
        "stock-torch sequence over the whole cache, or the library's causal grouped-query flash kernel (fp32 scores, no score "
        "tensor, the prefill independent of the cache length; opt-in: other logits, fidelity on the real checkpoint is unmeasured)"))
    p.add_argument("--caption_decode", choices=CAPTION_DECODES, default="valu", help="kernels of the token loop's weight-streaming products: " + (
        "on the vector ALU, or on MFMAs, whose arithmetic does not grow with --caption_batch (opt-in: other logits; the captions "
        "of --caption_batch N stay those of N = 1 inside the mode; see DESIGN.md section 8)" if batch else
        "on the vector ALU, or on MFMAs (another summation order: other logits, within the fp32 summation error; opt-in: "
        "fidelity on the real checkpoint is unmeasured)"))
    p.add_argument("--caption_attention", choices=CAPTION_ATTENTIONS, default="valu", help="attention of the token loop: " + (
        "on the vector ALU, or on MFMAs with key tiles by LDS-DMA (opt-in: other logits; the captions of --caption_batch N stay "
        "those of N = 1 inside the mode; see DESIGN.md section 8)" if batch else
        "on the vector ALU, or on MFMAs with key tiles by LDS-DMA (fp32 scores and a 16-bit P instead of 16-bit scores and an fp32 "
        "P: other logits; opt-in: fidelity on the real checkpoint is unmeasured)"))
    if batch:
        p.add_argument("--caption_batch", type=int, default=1, choices=range(1, 9), metavar="N", help="caption the Stage-1 images of N (1..8) "
                       "inputs in one token loop (the captioner's weights are streamed once per token for all of them); the same captions "
                       "and PNGs as N = 1 for a fixed --seed")


# ------------------------------------------------------------------------------------------------ image side (host)
def _resolutions(grid_pinpoints, patch_size):
    """``image_grid_pinpoints`` as a list of (width, height): a list, its string form, or the "(1x1),...,(3x3)" range form."""
    if isinstance(grid_pinpoints, str) and "x" in grid_pinpoints:
        spans = [(int(a), int(b)) for a, b in re.findall(r"\((\d+)x(\d+)\)", grid_pinpoints)]
        (a0, b0), (a1, b1) = spans[0], spans[-1]
        return [[i * patch_size, j * patch_size] for i in range(a0, a1 + 1) for j in range(b0, b1 + 1)]
    return grid_pinpoints if isinstance(grid_pinpoints, list) else ast.literal_eval(grid_pinpoints)


def select_best_resolution(original_size, possible_resolutions):
    """The candidate (width, height) that keeps most of the image's pixels after an aspect-preserving fit, ties broken by
    the least wasted canvas (mm_utils.py:121-151)."""
    ow, oh = original_size
    best, best_key = None, None
    for w, h in possible_resolutions:
        s = min(w / ow, h / oh)
        eff = min(int(ow * s) * int(oh * s), ow * oh)
        key = (eff, -(w * h - eff))
        if best_key is None or key > best_key:
            best, best_key = (w, h), key
    return best


def fit_and_offset(original_size, target_resolution):
    """The geometry of ``resize_and_pad_image`` -> ``(nw, nh, ox, oy)``: the aspect-preserving size of an image of ``original_size``
    = (width, height) inside ``target_resolution`` and where its top-left corner lands on the canvas (mm_utils.py:154-190)."""
    ow, oh = original_size
    tw, th = target_resolution
    sw, sh = tw / ow, th / oh
    if sw < sh:
        nw, nh = tw, min(math.ceil(oh * sw), th)
    else:
        nw, nh = min(math.ceil(ow * sh), tw), th
    return nw, nh, (tw - nw) // 2, (th - nh) // 2


def resize_and_pad_image(image, target_resolution):
    """Aspect-preserving resize (PIL default filter, like the reference) centred on a black canvas (mm_utils.py:154-190)."""
    from PIL import Image
    nw, nh, ox, oy = fit_and_offset(image.size, target_resolution)
    canvas = Image.new("RGB", tuple(target_resolution), (0, 0, 0))
    canvas.paste(image.resize((nw, nh)), (ox, oy))
    return canvas


def _proc_sizes(processor):
    """(shortest_edge, crop) of a CLIP image processor across transformers versions (dict, SizeDict or int pair)."""
    def get(obj, key):
        try:
            return obj[key]
        except (KeyError, TypeError, IndexError):
            return getattr(obj, key, None)
    size, crop = processor.size, processor.crop_size
    edge = get(size, "shortest_edge")
    if edge is None:
        edge = min(v for v in (get(size, "height"), get(size, "width")) if v is not None) if not isinstance(size, (tuple, list)) \
            else min(size)
    return int(edge), int(get(crop, "height"))


def process_anyres_image(image, processor, grid_pinpoints):
    """-> ``[1 + tiles, 3, S, S]``: the whole image squashed to S x S (the reference resizes, it does not pad,
    mm_utils.py:281-293), then the row-major S x S tiles of the best-fitting padded canvas."""
    edge, crop = _proc_sizes(processor)
    canvas = resize_and_pad_image(image, select_best_resolution(image.size, _resolutions(grid_pinpoints, edge)))
    w, h = canvas.size
    views = [image.resize((edge, edge))]
    views += [canvas.crop((x, y, x + crop, y + crop)) for y in range(0, h, crop) for x in range(0, w, crop)]
    return torch.stack([processor.preprocess(v, return_tensors="pt")["pixel_values"][0] for v in views], dim=0)


def process_images(images, image_processor, model_cfg):
    """mm_utils.py:316-340 for the aspect modes the shipped LLaVA-NeXT checkpoints use ("anyres"; plain preprocess otherwise)."""
    mode = getattr(model_cfg, "image_aspect_ratio", None)
    if mode == "anyres" or (mode is not None and "anyres_max" in mode):
        out = [process_anyres_image(im, image_processor, model_cfg.image_grid_pinpoints) for im in images]
        return torch.stack(out, dim=0) if all(o.shape == out[0].shape for o in out) else out
    if mode in ("highres", "crop_split", "pad"):
        raise NotImplementedError(f"image_aspect_ratio={mode!r}: the LLaVA-NeXT checkpoints of the pipeline use 'anyres'")
    return image_processor.preprocess(images, return_tensors="pt")["pixel_values"]


def process_images_device(u8_images, image_processor, model_cfg, dtype=torch.float16, plan=None):
    """``process_images`` of device uint8 HWC RGB images, on their device (``imageops.caption_views``: Pillow's resizes and the view
    assembly as kernels) -> the same views ``.to(dtype)``, bit for bit.  The anyres modes only: any other mode raises."""
    mode = getattr(model_cfg, "image_aspect_ratio", None)
    if not (mode == "anyres" or (mode is not None and "anyres_max" in mode)):
        raise NotImplementedError(f"image_aspect_ratio={mode!r}: the device route makes 'anyres' views only (and has no host fallback)")
    from . import imageops
    out = [imageops.caption_views(u8, image_processor, model_cfg.image_grid_pinpoints, dtype, plan) for u8 in u8_images]
    return torch.stack(out, dim=0) if all(o.shape == out[0].shape for o in out) else out


def anyres_grid_shape(image_size, grid_pinpoints, patch_size):
    """(tiles across, tiles down) of the canvas chosen for ``image_size`` = (width, height) (mm_utils.py:215-242)."""
    w, h = select_best_resolution(image_size, _resolutions(grid_pinpoints, patch_size))
    return w // patch_size, h // patch_size


def unpad_image(feat, original_size):
    """Crop a ``[C, H, W]`` feature map of a padded canvas back to the image's aspect (llava_arch.py:129-161; note the
    truncating ``int`` and the symmetric crop, which can leave one padded row / column)."""
    ow, oh = original_size
    ch, cw = feat.shape[1:]
    if ow / oh > cw / ch:                       # padded above / below
        pad = (ch - int(oh * (cw / ow))) // 2
        return feat[:, pad:ch - pad, :]
    pad = (cw - int(ow * (ch / oh))) // 2       # padded left / right
    return feat[:, :, pad:cw - pad]


# ------------------------------------------------------------------------------------------------ text side (host)
def tokenizer_image_token(prompt, tokenizer, image_token_index=IMAGE_TOKEN_INDEX, return_tensors=None):
    """Tokenise around every "<image>" and put ``image_token_index`` in its place; a BOS the tokenizer prepends to each
    chunk is kept once (mm_utils.py:343-362)."""
    chunks = [tokenizer(c).input_ids for c in prompt.split(DEFAULT_IMAGE_TOKEN)]
    has_bos = bool(chunks and chunks[0] and chunks[0][0] == tokenizer.bos_token_id)
    ids = [chunks[0][0]] if has_bos else []
    skip = 1 if has_bos else 0
    for i, c in enumerate(chunks):
        if i > 0:
            ids.append(image_token_index)
        ids.extend(c[skip:])
    if return_tensors is None:
        return ids
    if return_tensors != "pt":
        raise ValueError(f"Unsupported tensor type: {return_tensors}")
    return torch.tensor(ids, dtype=torch.long)


def llama3_prompt(tokenizer, question, system=LLAMA3_SYSTEM):
    """The prompt ``conv_templates["llava_llama_3"]`` builds for one user turn (conversation.py:98-110): the tokenizer's own
    chat template over [system, user], with the generation header appended."""
    messages = [{"role": "system", "content": system}, {"role": "user", "content": question}]
    return tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)


class _Llama3Template:
    """Minimal stand-in for an entry of the reference's ``conv_templates`` dict, for callers that pass one through
    ``get_img_describe(conv_templates=...)``."""
    system, roles = LLAMA3_SYSTEM, ("user", "assistant")


conv_templates = {"llava_llama_3": _Llama3Template()}


# ------------------------------------------------------------------------------------------------ the model
def _llama_config_cls():
    from transformers import LlamaConfig

    class LlavaNextConfig(LlamaConfig):
        model_type = "llava_llama"          # what config.json of the reference checkpoints says (llava_llama.py:30-37)

    return LlavaNextConfig


class _VisionTower(nn.Module):
    """``model.vision_tower``: holds the CLIP vision model as ``.vision_tower`` like the reference's CLIPVisionTower, and
    returns the hidden states of ``select_layer`` without the class token (clip_encoder.py:48-82)."""

    def __init__(self, clip, select_layer, select_feature):
        super().__init__()
        self.vision_tower = clip
        self.select_layer, self.select_feature = select_layer, select_feature
        if select_feature not in ("patch", "cls_patch"):
            raise NotImplementedError(f"mm_vision_select_feature={select_feature!r}")

    @property
    def config(self):
        return self.vision_tower.config

    @property
    def image_size(self):
        return self.config.image_size

    @property
    def num_patches_per_side(self):
        return self.config.image_size // self.config.patch_size

    def forward(self, images):
        p = next(self.vision_tower.parameters())
        hs = self.vision_tower(images.to(device=p.device, dtype=p.dtype), output_hidden_states=True).hidden_states[self.select_layer]
        return (hs[:, 1:] if self.select_feature == "patch" else hs).to(images.dtype)


def build_model(config, clip=None):
    """``LlavaNextLlama(config)``.  ``config``: a LlamaConfig carrying the reference's multimodal fields (mm_vision_tower,
    mm_projector_type, mm_hidden_size, mm_vision_select_layer, image_aspect_ratio, image_grid_pinpoints,
    mm_patch_merge_type).  ``clip``: a ready CLIPVisionModel, else one is built from ``config.mm_vision_tower``'s config."""
    from transformers import CLIPVisionConfig, CLIPVisionModel, LlamaForCausalLM

    class LlavaNextLlama(LlamaForCausalLM):
        config_class = _llama_config_cls()

        def __init__(self, cfg):
            super().__init__(cfg)
            tower = clip if clip is not None else CLIPVisionModel(CLIPVisionConfig.from_pretrained(cfg.mm_vision_tower))
            tower.requires_grad_(False)
            self.model.vision_tower = _VisionTower(tower, cfg.mm_vision_select_layer, getattr(cfg, "mm_vision_select_feature", "patch"))
            m = re.match(r"^mlp(\d+)x_gelu$", getattr(cfg, "mm_projector_type", "linear"))
            if m is None and cfg.mm_projector_type != "linear":
                raise NotImplementedError(f"mm_projector_type={cfg.mm_projector_type!r}")
            layers = [nn.Linear(cfg.mm_hidden_size, cfg.hidden_size)]
            for _ in range(1, int(m.group(1)) if m else 1):
                layers += [nn.GELU(), nn.Linear(cfg.hidden_size, cfg.hidden_size)]
            self.model.mm_projector = nn.Sequential(*layers) if m else layers[0]
            if "unpad" in getattr(cfg, "mm_patch_merge_type", ""):
                self.model.image_newline = nn.Parameter(torch.zeros(cfg.hidden_size))

        # -------- image features -> one [tokens, hidden] block per image
        def encode_images(self, pixel_values):
            return self.model.mm_projector(self.model.vision_tower(pixel_values))

        def image_blocks(self, images, image_sizes):
            """``images``: list of ``[1 + tiles, 3, S, S]`` (or a 5-D stack).  Base view first, then the un-padded tile grid
            with a newline embedding closing every feature row (mm_patch_merge_type "spatial_unpad", llava_arch.py:339-409)."""
            cfg = self.config
            merge = getattr(cfg, "mm_patch_merge_type", "flat")
            views = [im if im.ndim == 4 else im.unsqueeze(0) for im in images]
            feats = torch.split(self.encode_images(torch.cat(views, dim=0)), [v.shape[0] for v in views])
            if merge == "flat":
                return [f.flatten(0, 1) for f in feats]
            if merge != "spatial_unpad":
                raise NotImplementedError(f"mm_patch_merge_type={merge!r}")
            side = self.model.vision_tower.num_patches_per_side
            nl = self.model.image_newline
            out = []
            for f, size in zip(feats, image_sizes):
                if f.shape[0] == 1:
                    out.append(torch.cat([f[0], nl[None].to(f.dtype)], dim=0))
                    continue
                nx, ny = anyres_grid_shape(size, cfg.image_grid_pinpoints, self.model.vision_tower.image_size)
                grid = f[1:].view(ny, nx, side, side, -1).permute(4, 0, 2, 1, 3).reshape(f.shape[-1], ny * side, nx * side)
                grid = unpad_image(grid, size)
                grid = torch.cat([grid, nl.to(grid.dtype)[:, None, None].expand(-1, grid.shape[1], 1)], dim=-1)
                out.append(torch.cat([f[0], grid.flatten(1, 2).transpose(0, 1)], dim=0))
            return out

        def multimodal_embeds(self, input_ids, images, image_sizes):
            """``input_ids [1, T]`` holding IMAGE_TOKEN_INDEX placeholders -> ``inputs_embeds [1, T', hidden]``
            (llava_arch.py:440-497, single sequence, no padding)."""
            if input_ids.shape[0] != 1:
                raise NotImplementedError("the caption pass runs one prompt at a time (models/util.py:39-43)")
            ids = input_ids[0]
            blocks = self.image_blocks(images, image_sizes)
            where = (ids == IMAGE_TOKEN_INDEX).nonzero().flatten().tolist()
            if len(where) != len(blocks):
                raise ValueError(f"{len(where)} image placeholders in the prompt for {len(blocks)} images")
            embed = self.model.embed_tokens
            parts, start = [], 0
            for pos, blk in zip(where, blocks):
                parts += [embed(ids[start:pos]), blk.to(embed.weight.dtype)]
                start = pos + 1
            parts.append(embed(ids[start:]))
            emb = torch.cat(parts, dim=0)
            limit = getattr(self.config, "tokenizer_model_max_length", None)
            return emb[:limit][None]

        @torch.no_grad()
        def generate(self, inputs=None, images=None, image_sizes=None, **kw):
            """``generate(input_ids, images=[...], image_sizes=[(w, h)], do_sample=..., ...)`` like the reference's override
            (llava_llama.py:118-137): the prompt is handed to the decoder as embeddings."""
            kw.pop("modalities", None)
            if images is None:
                return super().generate(inputs, **kw)
            return super().generate(inputs_embeds=self.multimodal_embeds(inputs, images, image_sizes), **kw)

    return LlavaNextLlama(config)


class FastDecoder:
    """Token loop of the caption pass over a static key/value cache, with the decode step replayed from a hipGraph.

    ``transformers``' ``generate`` launches ~500 kernels per token from Python (8 B Llama: 32 layers) and is host-bound at
    20-30 ms per token; a caption is 256 tokens.  This class runs the SAME module weights (``model.model.layers[i].self_attn
    .{q,k,v,o}_proj``, ``.mlp.{gate,up,down}_proj``, the two RMSNorms, ``model.model.rotary_emb``, ``lm_head``) through a
    functional forward written out in stock torch ops -- RMSNorm, rotary embedding (half-split form), grouped-query SDPA
    over a pre-allocated ``[1, kv_heads, max_len, head_dim]`` cache, SwiGLU -- so that one decode step has static shapes
    and addresses and can be captured once (``torch.cuda.CUDAGraph`` = hipGraph) and replayed per token.  Sampling follows
    ``generate`` exactly (temperature, then one ``torch.multinomial`` per step; greedy = argmax), which is what
    tests/test_llava_next.py pins token for token against the reference's generations.  On the CPU (tests) the same code
    runs eagerly.

    ``weights``: "native" (default) streams the checkpoint's 16-bit weights.  "e4m3" (opt-in) packs the fused q|k|v, ``o_proj``,
    gate|up, ``down_proj`` and ``lm_head`` once as OCP e4m3 bytes with one power-of-two scale per output row (``rsvld_amd.w8``) and the
    fused decode step streams THOSE -- half the bytes of a loop bound by nothing else; activations, the KV cache, accumulation, the
    fused neighbours and sampling are unchanged.  The prefill keeps the 16-bit weights, so the packs come ON TOP of them: 8 GB beside
    the 16 GB that stay resident for the 8 B decoder (unless ``prefill_weights="e4m3"`` / ``release_native``, below).  The mode needs
    the fused decode step (``_fused_ok``) and ``K % 16 == 0`` in every packed product; where either fails the decoder raises -- it
    never falls back to the native weights silently.

    ``batch``: 1 (default) is the decoder described above.  ``batch=B`` (<= 8, opt-in) allocates ``[B, kv_heads, max_len, head_dim]`` caches
    and adds ``generate_batch``: up to ``B`` captions in ONE token loop, the weights streamed once per step for all of them
    (``rsvld_amd.decode_rows``), each caption token for token what ``generate`` gives for its prompt alone; ``generate`` itself keeps
    working on such a decoder (in cache row 0).

    ``prefill``: "torch" (default) is the prefill described above: the prompt's queries against the whole cache under an additive mask.
    "flash" (opt-in) runs the prefill's attention through the library's causal grouped-query flash kernel
    (``rsvld_amd.prefill_attention``): fp32 scores that are never rounded to 16 bits, no score or mask tensor, and a query row reads keys
    ``0 .. its own position`` only -- so the prefill's logits and cache rows do not depend on ``max_len`` or on what an earlier prompt
    left in the cache.  Other logits than "torch" gives (closer to an fp32 run, tests/test_gpu_caption_prefill.py); the projections,
    the rotary embedding, the cache write, the decode step and sampling are unchanged.  It needs 16-bit tensors on the GPU, head_dim
    128 and at most eight query heads per kv head; anything else raises -- it never falls back to "torch" silently.

    ``prefill_weights``: "native" (default) is the prefill described above, on the 16-bit weights.  "e4m3" (opt-in, requires
    ``weights="e4m3"``) sends the prefill's q|k|v, ``o_proj``, gate|up and ``down_proj`` through ``w8.linear_w8`` on the token loop's
    packs and the last row's ``lm_head`` through ``w8.gemv_w8``: the caption is then ONE model from the first prompt token on -- the
    torch model on ``w8.dequant(pack(w))`` up to summation order -- a prefill row's projections do not depend on the rows around it, and
    nothing reads the 16-bit decoder weights any more.
    ``release_native=True`` (requires ``prefill_weights="e4m3"``) therefore lets them go: packing proceeds layer by layer, a layer's
    seven projection weights are replaced by empty tensors once its four packs exist, ``lm_head.weight`` at the end (kept where it
    shares ``embed_tokens``' storage).  The packs are parked on the model (``model._e4m3_packs``); a decoder built later adopts them.
    On such a model every ``FastDecoder`` that needs the 16-bit weights, and ``merge_lora``, raise: reload the model.

    ``decode``: "valu" (default) runs the products of the fused decode step on the vector ALU (csrc/gemv.hip), whose per-row fp32
    arithmetic binds from four rows on.  "mfma" (opt-in) sends the four products per layer and ``lm_head`` through the MFMA kernels
    (csrc/gemv_mma.hip, ``decode_rows.gemv_rows(..., kernel="mfma")``) at EVERY row count, ``generate``'s single row included -- so
    that, inside the mode, ``generate_batch`` still equals ``generate`` per prompt token for token (a row's bits do not depend on the
    row count).  An MFMA sums in another order than the fmaf chain: other logits than "valu" gives, within the summation error of
    either.  Attention, the prefill and sampling are untouched; it combines with every other switch.  The mode needs the fused decode
    step (``_fused_ok``); where that fails the decoder raises -- it never falls back to "valu" or to torch silently.

    ``decode_attention``: "valu" (default) runs the decode step's attention through da_kernel (csrc/decode_attention.hip).  "mfma" (opt-in) sends it
    through dam_kernel of the same unit (``decode_rows.llama_decode_attention_rows(..., kernel="mfma")``) at EVERY row count,
    ``generate``'s single row included, so that inside the mode ``generate_batch`` still equals ``generate`` per prompt: key and value
    tiles by LDS-DMA, scores and P V on MFMAs, fp32 scores and a 16-bit P where "valu" has 16-bit scores and an fp32 P -- other logits,
    the same cache rows bit for bit.  It combines with every other switch and, like ``decode="mfma"``, needs the fused decode step
    (``_fused_ok``): where that fails the decoder raises.

    The six switches are ONE frozen record, ``self.mode`` (a ``CaptionMode``, which checks every value and combination that needs no
    model); ``weights`` .. ``decode_attention`` read it.  The weights are ONE table: per layer the products ``qkv``, ``o``, ``gu``, ``down``, then
    ``head``, each a ``(w, b, pack)`` -- the 16-bit weight, the bias, the e4m3 pack, None where the mode has none -- which
    ``_prefill_product`` and ``_step_product`` take."""

    WEIGHTS, PREFILLS, PREFILL_WEIGHTS, DECODES = CaptionMode.WEIGHTS, CAPTION_PREFILLS, CaptionMode.PREFILL_WEIGHTS, CAPTION_DECODES

    MAX_BATCH = 8            # RSVLD_DECODE_MAX_ROWS
    PARKED = "_e4m3_packs"   # the model attribute (plain, like ``_fast_decoder``) that holds the packs of a model whose 16-bit weights are released

    Product = collections.namedtuple("Product", "w b pack")            # one matrix product: 16-bit weight | None, bias | None, (q, scale) | None
    LayerProducts = collections.namedtuple("LayerProducts", "qkv o gu down")

    weights, prefill, prefill_weights, release_native, decode, decode_attention = (
        property(lambda self, f=f: getattr(self.mode, f))
        for f in ("weights", "prefill", "prefill_weights", "release_native", "decode", "decode_attention"))

    def __init__(self, model, max_len, weights="native", batch=1, prefill="torch", prefill_weights="native", release_native=False,
                 decode="valu", decode_attention="valu"):
        mode = CaptionMode(weights, prefill, prefill_weights, bool(release_native), decode, decode_attention)
        if not isinstance(batch, int) or not 1 <= batch <= self.MAX_BATCH:
            raise ValueError(f"FastDecoder: batch={batch!r}, expected 1..{self.MAX_BATCH}")
        parked = model.__dict__.get(self.PARKED)
        if parked is not None and (weights != "e4m3" or prefill_weights != "e4m3"):
            raise RuntimeError(f"FastDecoder(weights={weights!r}, prefill_weights={prefill_weights!r}): this model's 16-bit decoder weights "
                               f"were released by an earlier FastDecoder(release_native=True) and only its e4m3 packs remain; reload the "
                               f"model to run on the 16-bit weights")
        # (a model that is released stays so: its packs are adopted).  Assign a ``dataclasses.replace(dec.mode, ...)`` to switch a live
        # decoder between modes its table serves (tools/bench_caption_e4m3_only.py: ``prefill_weights`` is read by ``forward`` alone).
        self.mode = dataclasses.replace(mode, release_native=True) if parked is not None else mode
        self.batch = batch
        self._row = 0            # the cache row ``forward`` reads and writes (``generate_batch`` prefills row after row)
        self._rows = {}          # generate_batch: number of sequences -> the captured step (static buffers + graph)
        self._ws_rows = None
        cfg = model.config
        self.model, self.max_len = model, int(max_len)
        self.layers = list(model.model.layers)
        self.n_q, self.n_kv = cfg.num_attention_heads, cfg.num_key_value_heads
        self.hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        p = next(model.parameters())
        self.dev, self.dt = p.device, p.dtype
        if prefill == "flash" and not (self.dev.type == "cuda" and self.dt in (torch.float16, torch.bfloat16) and self.hd == 128
                                       and self.n_q % self.n_kv == 0 and self.n_q // self.n_kv <= 8):
            raise ValueError(f"FastDecoder(prefill='flash'): a {self.dt} model on {self.dev} with head_dim {self.hd} and {self.n_q} heads on "
                             f"{self.n_kv} kv heads is not covered by the flash prefill kernel (16-bit weights on the GPU, head_dim 128, at "
                             f"most 8 query heads per kv head are required; there is no fallback to 'torch')")
        shape = (batch, self.n_kv, self.max_len, self.hd)
        self.k = [torch.zeros(shape, device=self.dev, dtype=self.dt) for _ in self.layers]
        self.v = [torch.zeros(shape, device=self.dev, dtype=self.dt) for _ in self.layers]
        self.cols = torch.arange(self.max_len, device=self.dev)
        self._graph = None
        self.fused = True        # the decode step through the fused kernels where their conditions hold (``_fused_ok``); False = the torch-op sequence
        self.profile = None      # a dict: generate() fills in device-synchronised seconds of its prefill and its token loop
        self._build_table(parked)

    def _build_table(self, parked):
        """``self.table`` (a ``LayerProducts`` per layer), ``self.head`` and ``self._packs`` (the packs alone: a 4-tuple per layer, then
        the head's -- what is parked on a released model) in one pass over the layers.  Three questions shape a product: are parked
        packs ADOPTED (a decoder on a model an earlier one released: the parked packs ARE the weights), is it PACKED
        (``weights="e4m3"``), are its sources RELEASED.

        One weight-streaming GEMV for q | k | v and one for gate | up: the three (two) weight matrices of a layer become views of one
        concatenated tensor (no copy is kept, ``state_dict`` is unchanged), so a decode step launches 4 GEMVs per layer instead of 7.
        ``release_native``: product by product -- fuse, pack, then replace the sources by empty tensors -- so allocated memory never stands
        more than one layer's sources above the packs made so far; ``lm_head`` last (kept where it shares ``embed_tokens``' storage: a
        tied head is packed too, only not released).  The packs are parked on the model, where a decoder built later (a longer cache,
        more rows) finds them: their sources no longer exist."""
        head, emb = self.model.lm_head, self.model.model.embed_tokens.weight
        if parked is not None:
            if any(p.numel() for p in self._released_params()) or len(parked) != len(self.layers) + 1 or parked[-1][0].device != emb.device:
                raise RuntimeError("FastDecoder: this model's 16-bit decoder weights were released and its e4m3 packs no longer match it (a "
                                   "parameter was assigned since, or the model was moved); reload the model")
        elif self.weights == "e4m3":
            for t in dict.fromkeys(self._released_params() + [head.weight]):     # every source is checked before the first one is packed or released
                self._packable(t)
        if any(layer.mlp.gate_proj.bias is not None for layer in self.layers):
            raise NotImplementedError("FastDecoder: biased MLP projections")
        tied = head.weight.untyped_storage().data_ptr() == emb.untyped_storage().data_ptr()
        self.table = []
        with torch.no_grad():
            for i, layer in enumerate(self.layers):
                at, mlp = layer.self_attn, layer.mlp
                qkv = (at.q_proj, at.k_proj, at.v_proj)
                b_qkv = self._fuse(qkv, "bias") if at.q_proj.bias is not None else None
                sources = ((qkv, b_qkv), ((at.o_proj,), at.o_proj.bias), ((mlp.gate_proj, mlp.up_proj), None), ((mlp.down_proj,), None))
                adopted = parked[i] if parked is not None else [None] * len(sources)
                self.table.append(self.LayerProducts(*(self._product(mods, b, pack) for (mods, b), pack in zip(sources, adopted))))
            self.head = self._product((head,), head.bias, parked[-1] if parked is not None else None, release=not tied)
        if parked is not None:
            self._packs = parked
        elif self.weights == "e4m3":
            self._packs = [tuple(p.pack for p in row) for row in self.table] + [self.head.pack]
            if self.release_native:
                self.model.__dict__[self.PARKED] = self._packs       # not a submodule, not a buffer: a plain attribute
            else:   # what ``stale`` compares: a pack is a COPY, so an in-place update of its source (a LoRA merge) must be seen too
                self._pack_state = [self._identity(t) for t in self._pack_sources()]
        else:
            self._packs = None

    def _product(self, mods, bias, adopted, release=True):
        """The ``Product`` of one module, or of several fused into one (their weights become views of the concatenation)."""
        if adopted is not None:
            return self.Product(None, bias, adopted)
        w = self._fuse(mods, "weight") if len(mods) > 1 else mods[0].weight
        if self.weights != "e4m3":
            return self.Product(w, bias, None)
        if not self.release_native:
            from . import w8
            return self.Product(w, bias, w8.pack_rows_e4m3(w.contiguous()))
        pack = self._pack_tight(w.contiguous())
        del w                                                # (the fused tensor goes with the views the modules held)
        if release:
            self._release(*mods)
        return self.Product(None, bias, pack)

    # ------------------------------------------------------------------ release_native: the packs are the only copy of the decoder's weights
    def _released_params(self):
        """The parameters ``release_native`` empties: the seven projection weights of every layer, then ``lm_head.weight`` unless it
        shares ``embed_tokens``' storage (a tied head stays: the embedding reads it)."""
        ps = []
        for layer in self.layers:
            at, mlp = layer.self_attn, layer.mlp
            ps += [m.weight for m in (at.q_proj, at.k_proj, at.v_proj, at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj)]
        head, emb = self.model.lm_head.weight, self.model.model.embed_tokens.weight
        tied = head.numel() > 0 and head.untyped_storage().data_ptr() == emb.untyped_storage().data_ptr()
        return ps if tied else ps + [head]

    @staticmethod
    def _pack_tight(w):
        """``w8.pack_rows_e4m3(w)`` with the bytes in an allocator block of exactly their size.  torch's caching allocator hands a
        request the smallest free block that holds it and does not split the block when 1 MiB or less would remain -- and a release
        leaves exactly such holes (a 1.5 MiB pack falls into the 2 MiB a source just left and keeps, and counts as, all of it): up to
        1 MiB per pack of memory that was to be freed.  So the size is probed first: a probe that came with more than its own bytes is
        held back (its hole is then out of the way) and the next one tried; the probe that fits alone is freed, and the pack's
        allocation, the same size on the same stream, takes the block it leaves (an exact fit is the smallest block that holds it).
        After the holes the allocator cuts from a large block or a fresh segment, which is exact; the held holes are freed again.
        How many holes there are depends on what the process did before (networks that pack lazily leave their packs between the
        activations of their first forward, and the gaps stay when they are freed): the bound only ends the search, it is not expected
        to be reached (8 was: the figure of tests/test_gpu_caption_e4m3_only.py stood 21 184 bytes above its bound behind the suite)."""
        from . import w8
        dev, nbytes = w.device, w.numel()                  # one e4m3 byte per weight
        exact = -(-nbytes // 512) * 512                      # the allocator's own rounding
        held, probe = [], None
        for _ in range(64):
            before = torch.cuda.memory_allocated(dev)
            probe = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if torch.cuda.memory_allocated(dev) - before <= exact:
                break
            held.append(probe)
        del probe
        packed = w8.pack_rows_e4m3(w)
        del held
        return packed

    @staticmethod
    def _release(*mods):
        for m in mods:
            m.weight.data = torch.empty(0, dtype=m.weight.dtype, device=m.weight.device)

    @staticmethod
    def _packable(t):
        if t.dim() != 2 or t.shape[1] % 16 or t.dtype not in (torch.float16, torch.bfloat16) or not t.is_cuda:
            raise ValueError(f"FastDecoder(weights='e4m3'): a {t.dtype} weight of shape {tuple(t.shape)} on {t.device} cannot be "
                             f"packed (16-bit weights on the GPU with K % 16 == 0 are required; there is no fallback to 'native')")

    def _pack_sources(self):
        """The 16-bit tensors the e4m3 mode packs, in pack order: per layer q|k|v, o_proj, gate|up, down_proj; then lm_head."""
        src = []
        for row, layer in zip(self.table, self.layers):
            src += [row.qkv.w, layer.self_attn.o_proj.weight, row.gu.w, layer.mlp.down_proj.weight]
        return src + [self.model.lm_head.weight]

    @staticmethod
    def _identity(t):
        """(storage address, in-place version) of a packed source; an inference-mode tensor counts no versions."""
        try:
            return t.data_ptr(), t._version
        except RuntimeError:
            return t.data_ptr(), 0

    def stale(self):
        """The fused q | k | v and gate | up tensors are VIEWED by the model's own modules; ``model.to()`` / ``.half()`` / a LoRA merge /
        ``load_state_dict(assign=True)`` give the modules new storage and leave this decoder (weights, KV cache, captured graph) on
        the old one.  Cheap check: first and last layer still alias the fused tensors, on the same device and dtype.
        ``release_native``: there is nothing left to alias -- stale when a released parameter holds elements again (the model was
        reloaded under the decoder) or the packs sit on another device than ``embed_tokens``."""
        if self.release_native:
            return (any(p.numel() for p in self._released_params())
                    or self._packs[-1][0].device != self.model.model.embed_tokens.weight.device)
        for i in (0, len(self.layers) - 1):
            q, wqkv = self.layers[i].self_attn.q_proj.weight, self.table[i].qkv.w
            g, wgu = self.layers[i].mlp.gate_proj.weight, self.table[i].gu.w
            if q.data_ptr() != wqkv.data_ptr() or g.data_ptr() != wgu.data_ptr() or q.device != wqkv.device or q.dtype != wqkv.dtype:
                return True
        if self._packs is not None:      # the e4m3 packs are copies: same storage, not written since, and on the weights' device
            src = self._pack_sources()
            if [self._identity(t) for t in src] != self._pack_state or self._packs[-1][0].device != src[-1].device:
                return True
        return False

    @staticmethod
    def _fuse(mods, name):
        with torch.no_grad():
            parts = [getattr(m, name) for m in mods]
            fused = torch.cat([q.data for q in parts], dim=0)
            o = 0
            for q in parts:
                q.data = fused[o:o + q.shape[0]]      # the module keeps working (and saving) through a view of the fused tensor
                o += q.shape[0]
        return fused

    def _rms(self, x, norm):
        return torch.nn.functional.rms_norm(x, (x.shape[-1],), norm.weight, norm.variance_epsilon)

    def _lin(self, x, w, b=None):
        """``x [T, K] @ w[N, K]^T``.  The decode step (ONE row, 16-bit, on the GPU) streams the weights through this library's
        HBM-bound matrix-vector kernel (rsvld_gemv: the PyTorch GEMV of the same shapes ran at ~3 TB/s); everything else is
        ``torch.nn.functional.linear``."""
        if x.shape[0] == 1 and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and w.is_contiguous() and w.shape[1] % 8 == 0:
            from . import ops
            return ops.gemv(w, x[0].contiguous(), b)[None]
        return torch.nn.functional.linear(x, w, b)

    def _prefill_product(self, p, x):
        """``x [T, K]`` times product ``p`` in ``forward``.  ``prefill_weights="e4m3"``: on the token loop's pack -- the 16-bit weights
        are not read -- through the tile GEMM, and ONE row (the last position under ``lm_head``) through the matrix-vector product of the
        decode step; else ``_lin`` on the 16-bit weight."""
        if self.prefill_weights != "e4m3":
            return self._lin(x, p.w, p.b)
        from . import w8
        if x.shape[0] == 1:
            return w8.gemv_w8(*p.pack, x[0].contiguous(), p.b)[None]
        return w8.linear_w8(*p.pack, x.contiguous(), p.b)

    def _step_product(self, p, x, **fused):
        """``x [n, K]`` times product ``p`` in the fused decode step of ``n`` rows, on the pack where the decoder has packs, with the
        neighbours ``fused`` in (``norm=``, ``residual=``, ``glu=``), on the kernels of ``decode``."""
        from . import decode_rows as DR
        if p.pack is not None:
            return DR.gemv_w8_rows(*p.pack, x, p.b, kernel=self.decode, **fused)
        return DR.gemv_rows(p.w, x, p.b, kernel=self.decode, **fused)

    def forward(self, embeds, pos, pos0=None):
        """``embeds [1, T, H]`` at absolute positions ``pos [T]`` (long, on the device) -> logits of the LAST position
        ``[1, vocab]``; writes the keys / values of these positions into the cache.  One code path for the prefill (T > 1)
        and the decode step (T = 1): scores in the activation type, softmax in fp32 (``transformers``' eager attention),
        grouped-query heads as a batched matmul over the kv heads -- no expanded copy of the cache, no mask tensor beyond an
        additive ``[T, max_len]`` row.  ``prefill="flash"``, T > 1: the attention is ``prefill_attention.llama_prefill_attention`` (no
        mask tensor at all); ``pos`` must then be ``pos0, pos0 + 1, ..`` and the caller says ``pos0`` as a HOST int (``generate`` /
        ``generate_batch``: 0) -- it is not read back from ``pos``, which would be a host synchronisation."""
        m = self.model.model
        T = embeds.shape[1]
        nq, nkv, hd = self.n_q, self.n_kv, self.hd
        g = nq // nkv
        if T == 1 and self._fused_ok(embeds):
            return self._forward_fused(embeds, pos)
        if T == 1 and self.decode != "valu":
            raise RuntimeError(f"FastDecoder(decode={self.decode!r}): the fused decode step is not available for this model / input "
                               "(see _fused_ok) and the mode has no other path; use decode='valu'")
        if T == 1 and self.decode_attention != "valu":
            raise RuntimeError(f"FastDecoder(decode_attention={self.decode_attention!r}): the fused decode step is not available for this "
                               "model / input (see _fused_ok) and the mode has no other path; use decode_attention='valu'")
        if T == 1 and self._packs is not None:
            raise RuntimeError("FastDecoder(weights='e4m3'): the fused decode step is not available for this model / input "
                               "(see _fused_ok) and the e4m3 weights have no other path; use weights='native'")
        cos, sin = m.rotary_emb(embeds, pos[None])                                 # [1, T, hd]
        cos, sin = cos[0][:, None], sin[0][:, None]                                # [T, 1, hd]
        flash = self.prefill == "flash" and T > 1
        if flash:
            if pos0 is None:
                raise ValueError("FastDecoder(prefill='flash').forward: pos0 (the host int position of the first row) is required at T > 1")
            from . import prefill_attention as PA
        else:
            bias = torch.zeros((T, self.max_len), device=self.dev, dtype=torch.float32)
            bias.masked_fill_(self.cols[None, :] > pos[:, None], float("-inf"))   # causal over the filled prefix
        scale = hd ** -0.5
        h = embeds[0]                                                               # [T, H]
        lin = self._prefill_product
        for i, (layer, w) in enumerate(zip(self.layers, self.table)):
            x = self._rms(h, layer.input_layernorm)
            qkv = lin(w.qkv, x).view(T, nq + 2 * nkv, hd)
            qk = qkv[:, :nq + nkv]
            half = hd // 2
            qk = qk * cos + torch.cat((-qk[..., half:], qk[..., :half]), dim=-1) * sin     # rotary embedding on q and k at once
            kc, vc = self.k[i][self._row], self.v[i][self._row]
            kc.index_copy_(1, pos, qk[:, nq:].transpose(0, 1))
            vc.index_copy_(1, pos, qkv[:, nq + nkv:].transpose(0, 1))
            if flash:      # q stays the column slice of qk it is: the kernel takes its token stride
                o = PA.llama_prefill_attention(qk[:, :nq], kc, vc, nq, nkv, scale, pos0=int(pos0))
            else:
                q = qk[:, :nq].reshape(T, nkv, g, hd).permute(1, 0, 2, 3).reshape(nkv, T * g, hd)  # [kv head, (t, q-in-group), hd]
                sc = torch.matmul(q, kc.transpose(1, 2)).float().view(nkv, T, g, self.max_len)
                pr = torch.softmax(sc * scale + bias[None, :, None, :], dim=-1).to(self.dt).view(nkv, T * g, self.max_len)
                o = torch.matmul(pr, vc).view(nkv, T, g, hd).permute(1, 0, 2, 3).reshape(T, nq * hd)
            h = h + lin(w.o, o)
            x = self._rms(h, layer.post_attention_layernorm)
            gu = lin(w.gu, x)
            inter = gu.shape[-1] // 2
            h = h + lin(w.down, torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:])
        return lin(self.head, self._rms(h[-1:], m.norm))

    def _fused_ok(self, embeds):
        """The decode step as the library's fused kernels (rsvld_gemv_fused, rsvld_llama_decode_attention): 16-bit tensors on the GPU, head_dim
        128, at most eight query heads per kv head, unbiased MLP, 16-byte aligned rows (``weights="e4m3"``: of e4m3 too, K % 16 == 0 in every
        product -- checked when the packs are made)."""
        return (self.fused and embeds.is_cuda and embeds.dtype in (torch.float16, torch.bfloat16) and self.hd == 128
                and self.n_q % self.n_kv == 0 and self.n_q // self.n_kv <= 8 and embeds.shape[-1] % 8 == 0)

    def _forward_fused(self, embeds, pos):
        """ONE new token (``embeds [1, 1, H]``) of the sequence in cache row ``_row`` -> logits ``[1, vocab]``: ``_forward_rows`` on that row."""
        return self._forward_rows(embeds[0], pos, self._row)

    def _pick(self, logits, do_sample, temperature, top_k=0, top_p=1.0, generator=None):
        """``generate``'s sampling chain (transformers' TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial).
        The reference calls ``generate(do_sample=True, temperature=0.2)`` (models/util.py:50-60) and thereby inherits the generation
        config's ``top_k`` (transformers' default: 50): sampling the full softmax instead would be a different sampler."""
        if not do_sample:
            return logits.argmax(-1)
        scores = logits.float() / temperature
        if top_k and top_k > 0:
            kth = torch.topk(scores, min(int(top_k), scores.shape[-1]))[0][..., -1, None]
            scores = scores.masked_fill(scores < kth, float("-inf"))
        if top_p is not None and top_p < 1.0:
            srt, idx = torch.sort(scores, descending=False)
            remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - top_p)
            remove[..., -1:] = False                                   # min_tokens_to_keep = 1
            scores = scores.masked_fill(remove.scatter(-1, idx, remove), float("-inf"))
        return torch.multinomial(torch.softmax(scores, dim=-1), 1, generator=generator)[:, 0]

    def _sampling_defaults(self, do_sample, top_k, top_p):
        """``None`` = what ``generate`` would take from the model's generation_config for a sampling call (top_k 50, top_p 1.0 unless
        the checkpoint says otherwise)."""
        g = getattr(self.model, "generation_config", None)
        if top_k is None:
            top_k = getattr(g, "top_k", 50) if do_sample else 0
        if top_p is None:
            top_p = getattr(g, "top_p", 1.0) if do_sample else 1.0
        return (top_k or 0), (1.0 if top_p is None else top_p)

    @torch.no_grad()
    def generate(self, inputs_embeds, max_new_tokens, do_sample=False, temperature=1.0, eos_token_id=None, use_graph=None,
                 top_k=None, top_p=None):
        """-> ``[n]`` generated token ids (n <= max_new_tokens; stops after an ``eos_token_id``, which is included).
        ``top_k`` / ``top_p``: None = the generation config's values, as ``generate`` resolves them."""
        top_k, top_p = self._sampling_defaults(do_sample, top_k, top_p)
        T0 = inputs_embeds.shape[1]
        if T0 + max_new_tokens > self.max_len:
            raise ValueError(f"FastDecoder: prompt {T0} + {max_new_tokens} new tokens exceed the cache ({self.max_len})")
        use_graph = (self.dev.type == "cuda") if use_graph is None else use_graph
        eos = set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))
        embed = self.model.model.embed_tokens
        t_start = self._stamp()
        logits = self.forward(inputs_embeds.to(self.dt), torch.arange(T0, device=self.dev), pos0=0)
        tok = self._pick(logits, do_sample, temperature, top_k, top_p)
        out = [tok]
        t_prefill = self._stamp()
        if use_graph and self._graph is None:                          # (the warm-up rewrites cache slot T0 with the same values)
            self._tok, self._pos, self._logits, self._graph = self._capture(lambda e, p: self.forward(e[None], p), tok.clone(),
                                                                            torch.tensor([T0], device=self.dev))
        for n in range(1, max_new_tokens):
            if eos and int(tok) in eos:
                break
            if use_graph:
                self._tok.copy_(tok.view(-1))
                self._pos.fill_(T0 + n - 1)
                self._graph.replay()
                logits = self._logits
            else:
                logits = self.forward(embed(tok)[None], torch.tensor([T0 + n - 1], device=self.dev))
            tok = self._pick(logits, do_sample, temperature, top_k, top_p)
            out.append(tok)
        if self.profile is not None:
            self.profile.update(prompt_tokens=T0, prefill_s=t_prefill - t_start, decode_s=self._stamp() - t_prefill, new_tokens=len(out))
        return torch.cat(out)

    def _stamp(self):
        """``profile`` bookkeeping: the host time once this stream's work is done (this stream only: a caller may run other work on a
        second stream beside the token loop); None while no profile is asked for."""
        if self.profile is None:
            return None
        torch.cuda.current_stream().synchronize()
        return time.perf_counter()

    def _capture(self, step, tok, pos):
        """``step(embeddings of tok, pos)`` -- the decode step on the static buffers ``tok`` / ``pos`` -- warmed up on a side stream (off
        the capture stream: allocator, lazy init; it rewrites the cache slots at ``pos`` with the same values), then captured as ONE
        stream's linear chain of launches -> ``(tok, pos, logits, graph)``."""
        embed = self.model.model.embed_tokens
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(embed(tok), pos)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = step(embed(tok), pos)
        return tok, pos, logits, graph

    # ------------------------------------------------------------------ several captions in one token loop
    def _forward_rows(self, h, pos, row0=0):
        """The decode step of ``n`` sequences in 7 launches per layer instead of ~26: RMSNorm folded into the q|k|v and gate|up products, rotary
        embedding + cache write + grouped-query attention in one operator, the residual additions in the o_proj / down_proj epilogues, SwiGLU in
        down_proj's prologue.  Same arithmetic and the same roundings as ``forward`` up to the order of two fp32 sums (the RMSNorm's mean, the
        softmax over key chunks) and the 16-bit rounding of P, which this path skips.  ``h [n, H]`` = the embeddings of the sequences' newest
        tokens, ``pos [n]`` (long, on the device) their positions -> logits ``[n, vocab]``; the caches of rows ``row0 .. row0 + n - 1`` are
        updated at ``pos``.  The weights are streamed ONCE for all rows (``rsvld_amd.decode_rows``), and row ``b`` of every operator is bit
        for bit the operator on row ``b`` alone."""
        from . import decode_rows as DR
        m = self.model.model
        n = h.shape[0]
        cos, sin = m.rotary_emb(h[None], pos[None])                                # [1, n, hd]
        cos, sin = cos[0].contiguous(), sin[0].contiguous()
        h = h.contiguous()
        scale = self.hd ** -0.5
        if self._ws_rows is None:
            # ONE workspace for the decoder's life, sized for ``batch`` rows: the captured steps of ``_rows`` hold its address, so it is
            # never replaced (a buffer grown per row count would be freed under the graphs captured with fewer rows, ``_graph`` among
            # them).  Per-chunk partial results: written before they are read, no initial state.
            need = DR.decode_attention_ws_floats(self.n_q, self.n_kv, self.max_len, self.batch, self.decode_attention)
            self._ws_rows = torch.empty(need, device=self.dev, dtype=torch.float32)
        gemv = self._step_product
        for i, (layer, w) in enumerate(zip(self.layers, self.table)):
            n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
            qkv = gemv(w.qkv, h, norm=(n1.weight, n1.variance_epsilon))
            o = DR.llama_decode_attention_rows(qkv, cos, sin, pos, self.k[i][row0:row0 + n], self.v[i][row0:row0 + n], self.n_q, self.n_kv, scale,
                                               ws=self._ws_rows, kernel=self.decode_attention)
            h = gemv(w.o, o, residual=h)
            gu = gemv(w.gu, h, norm=(n2.weight, n2.variance_epsilon))
            h = gemv(w.down, gu, glu=True, residual=h)
        return gemv(self.head, h, norm=(m.norm.weight, m.norm.variance_epsilon))

    def _row_generators(self, n, seeds):
        if seeds is None:
            return [None] * n
        if len(seeds) != n:
            raise ValueError(f"FastDecoder.generate_batch: {len(seeds)} seeds for {n} prompts")
        return [torch.Generator(device=self.dev).manual_seed(int(s)) for s in seeds]

    @torch.no_grad()
    def generate_batch(self, inputs_embeds, max_new_tokens, do_sample=False, temperature=1.0, eos_token_id=None, seeds=None, use_graph=None,
                       top_k=None, top_p=None):
        """``generate`` for up to ``batch`` prompts (a list of ``[1, T_b, H]``, lengths may differ) in ONE token loop -> a list of token
        tensors, each EQUAL to what ``generate`` returns for that prompt alone: the prefill runs prompt after prompt through ``forward``
        into the prompt's cache row, the decode step of all rows runs through the multi-row operators (bit-identical per row), captured
        once per number of rows.  Sampling: row ``b`` draws from a generator of its own seeded ``seeds[b]`` -- the draws of the
        one-at-a-time call under ``torch.random.fork_rng`` + ``torch.manual_seed(seeds[b])``; the caller's generators are not touched
        (``seeds=None``: every row draws from the current default generator).  A row that has emitted an end token stops: its position
        is frozen and what the step computes for it is discarded; the loop ends when every row has.  Where the fused step is not
        available (a CPU decoder, ``_fused_ok``) the prompts go through ``generate`` one after another, with one warning."""
        n = len(inputs_embeds)
        if not 1 <= n <= self.batch:
            raise ValueError(f"FastDecoder.generate_batch: {n} prompts for a decoder built with batch={self.batch}")
        T0s = [int(e.shape[1]) for e in inputs_embeds]
        if max(T0s) + max_new_tokens > self.max_len:
            raise ValueError(f"FastDecoder: prompt {max(T0s)} + {max_new_tokens} new tokens exceed the cache ({self.max_len})")
        if seeds is not None and len(seeds) != n:
            raise ValueError(f"FastDecoder.generate_batch: {len(seeds)} seeds for {n} prompts")
        if not self._fused_ok(inputs_embeds[0].to(self.dt)):
            if self.decode != "valu":
                raise RuntimeError(f"FastDecoder(decode={self.decode!r}).generate_batch: the fused decode step is not available for this "
                                   "model / device (see _fused_ok) and the mode has no other path; use decode='valu'")
            if self.decode_attention != "valu":
                raise RuntimeError(f"FastDecoder(decode_attention={self.decode_attention!r}).generate_batch: the fused decode step is not "
                                   "available for this model / device (see _fused_ok) and the mode has no other path; use decode_attention='valu'")
            import warnings
            warnings.warn("FastDecoder.generate_batch: the fused decode step is not available for this model / device; the prompts are "
                          "captioned one after another (same tokens)")
            outs = []
            for b, e in enumerate(inputs_embeds):
                kw = dict(do_sample=do_sample, temperature=temperature, eos_token_id=eos_token_id, use_graph=use_graph, top_k=top_k, top_p=top_p)
                if seeds is None:
                    outs.append(self.generate(e, max_new_tokens, **kw))
                else:
                    with torch.random.fork_rng(devices=[self.dev] if self.dev.type == "cuda" else []):
                        torch.manual_seed(int(seeds[b]))
                        outs.append(self.generate(e, max_new_tokens, **kw))
            return outs
        top_k, top_p = self._sampling_defaults(do_sample, top_k, top_p)
        use_graph = True if use_graph is None else use_graph
        eos = set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))
        embed = self.model.model.embed_tokens
        gens = self._row_generators(n, seeds)
        t_start = self._stamp()
        first = []
        try:
            for b, e in enumerate(inputs_embeds):                      # prefill: matrix-bound, one prompt at a time, into cache row b
                self._row = b
                logits = self.forward(e.to(self.dt), torch.arange(T0s[b], device=self.dev), pos0=0)
                first.append(self._pick(logits, do_sample, temperature, top_k, top_p, generator=gens[b]))
        finally:
            self._row = 0
        toks = torch.cat(first)                                        # [n]
        pos = torch.tensor(T0s, device=self.dev)
        t_prefill = self._stamp()
        st = self._rows.get(n) if use_graph else None
        if use_graph and st is None:
            st = self._rows[n] = dict(zip(("tok", "pos", "logits", "graph"), self._capture(self._forward_rows, toks.clone(), pos.clone())))
        host = toks.tolist()
        out = [[t] for t in first]
        done = [bool(eos) and host[b] in eos for b in range(n)]
        live = torch.tensor([0 if d else 1 for d in done], device=self.dev)
        steps = 0
        for _ in range(1, max_new_tokens):
            if all(done):
                break
            if use_graph:
                st["tok"].copy_(toks)
                st["pos"].copy_(pos)
                st["graph"].replay()
                logits = st["logits"]
            else:
                logits = self._forward_rows(embed(toks), pos)
            if do_sample:                                              # row by row: the shapes, kernels and draws of the single call
                # (a finished row draws nothing: with ``seeds=None`` all rows share the caller's generator)
                new = torch.cat([toks[b:b + 1] if done[b] else self._pick(logits[b:b + 1], True, temperature, top_k, top_p, generator=gens[b])
                                 for b in range(n)])
            else:
                new = logits.argmax(-1)
            steps += 1
            toks = torch.where(live.bool(), new, toks)                 # a finished row keeps its last token and its position
            pos = pos + live
            host = new.tolist()
            changed = False
            for b in range(n):
                if not done[b]:
                    out[b].append(new[b:b + 1])
                    if eos and host[b] in eos:
                        done[b] = changed = True
            if changed:
                live = torch.tensor([0 if d else 1 for d in done], device=self.dev)
        if self.profile is not None:
            self.profile.update(prompt_tokens=T0s, prefill_s=t_prefill - t_start, decode_s=self._stamp() - t_prefill,
                                new_tokens=[len(o) for o in out], steps=steps, rows=n)
        return [torch.cat(o) for o in out]


def normalise_checkpoint_keys(state_dict, model):
    """Checkpoints written by transformers 4.x name the CLIP weights ``...vision_tower.vision_tower.vision_model.*``;
    transformers 5 modules drop the ``vision_model.`` level (and vice versa).  Rename towards what ``model`` has."""
    have = set(model.state_dict().keys())
    mid = ".vision_tower.vision_tower."
    out = {}
    for k, v in state_dict.items():
        if k not in have and mid in k:
            alt = k.replace(mid + "vision_model.", mid) if mid + "vision_model." in k else k.replace(mid, mid + "vision_model.")
            if alt in have:
                k = alt
        out[k] = v
    return out


def merge_lora(model, adapter_dir):
    """Fold a PEFT LoRA adapter (adapter_config.json + adapter_model.safetensors / .bin) into ``model``'s Linear weights:
    ``W += (B @ A) * lora_alpha / r``.  Equivalent to ``PeftModel.from_pretrained(...).merge_and_unload()`` for plain LoRA on
    Linear layers; anything else in the adapter raises."""
    if model.__dict__.get(FastDecoder.PARKED) is not None:
        raise RuntimeError("merge_lora: this model's 16-bit decoder weights were released (FastDecoder(release_native=True) / caption "
                           "weights 'e4m3-only') and there is nothing to merge into; reload the model, merge, then build the decoder")
    cfg = json.load(open(os.path.join(adapter_dir, "adapter_config.json")))
    if cfg.get("peft_type", "LORA") != "LORA" or cfg.get("use_dora") or cfg.get("modules_to_save"):
        raise NotImplementedError("merge_lora handles plain LoRA adapters on Linear layers")
    scale = cfg["lora_alpha"] / cfg["r"]
    st = os.path.join(adapter_dir, "adapter_model.safetensors")
    if os.path.exists(st):
        import safetensors.torch
        sd = safetensors.torch.load_file(st)
    else:
        sd = torch.load(os.path.join(adapter_dir, "adapter_model.bin"), map_location="cpu")
    mods = dict(model.named_modules())
    merged = 0
    for ka, a in sd.items():
        if ".lora_A" not in ka:
            if ".lora_B" not in ka:
                raise NotImplementedError(f"unexpected adapter tensor {ka}")
            continue
        name = re.sub(r"^base_model\.model\.", "", ka.split(".lora_A")[0])
        b = sd[ka.replace(".lora_A", ".lora_B")]
        lin = mods[name]
        lin.weight.data += (b.to(torch.float32) @ a.to(torch.float32)).to(lin.weight) * scale
        merged += 1
    return merged


def resolve_model_dir(model_path):
    """A local directory as is; a hub id (``lmms-lab/llama3-llava-next-8b``, models/util.py:112-114) through the local
    Hugging Face cache only -- this build never fetches from the network."""
    if os.path.isdir(model_path):
        return model_path
    try:
        from huggingface_hub import snapshot_download
        return snapshot_download(model_path, local_files_only=True)
    except Exception as exc:   # not cached (LocalEntryNotFoundError), malformed id, hub library absent
        raise FileNotFoundError(
            f"load_llava: {model_path!r} is neither a directory nor a snapshot in the local Hugging Face cache "
            f"({type(exc).__name__}); download the checkpoint first, or skip the captioner with --no_llava / --caption") from exc


def load_llava(device="cuda", model_path=DEFAULT_MODEL, adapter_path=DEFAULT_ADAPTER, dtype=torch.float16):
    """-> (tokenizer, model, image_processor), the tuple of models/util.py:111-117.  SDPA attention (flash-attn does not
    exist on this platform and is not needed); the adapter is applied by ``peft`` when installed, else merged here.
    The skeleton is built on the meta device (no 32 GB fp32 random init of an 8 B model on the host) and EVERY parameter
    and buffer must then come from the checkpoint: a tensor no shard supplies raises instead of staying random."""
    import glob

    import safetensors.torch
    from transformers import AutoTokenizer, CLIPImageProcessor
    model_dir = resolve_model_dir(model_path)
    cfg_cls = _llama_config_cls()
    config = cfg_cls.from_pretrained(model_dir)
    config._attn_implementation = "sdpa"
    tokenizer = AutoTokenizer.from_pretrained(model_dir, use_fast=False)
    shards = sorted(glob.glob(os.path.join(model_dir, "*.safetensors")))
    if not shards:
        raise FileNotFoundError(f"load_llava: no *.safetensors under {model_dir!r} (download the checkpoint there first; "
                                f"this build does not fetch from the network)")
    with torch.device("meta"):
        model = build_model(config)
    wanted = set(model.state_dict().keys())
    loaded = set()
    for sh in shards:
        sd = normalise_checkpoint_keys(safetensors.torch.load_file(sh), model)
        extra = [k for k in sd if k not in wanted]
        if extra:
            raise RuntimeError(f"load_llava: unexpected keys in {sh}: {extra[:5]}")
        model.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, strict=False, assign=True)
        loaded.update(sd.keys())
    # buffers that are derived, not stored (rotary inv_freq, CLIP position_ids) are re-created below; everything else
    # the checkpoint must hold
    missing = sorted(k for k in wanted - loaded if not k.endswith(("inv_freq", "position_ids")))
    if missing:
        raise RuntimeError(f"load_llava: {len(missing)} tensors of the model are in no shard of {model_dir!r} and would stay "
                           f"uninitialised, e.g. {missing[:5]} (vision tower / mm_projector / image_newline must be in the "
                           f"checkpoint, as in lmms-lab/llama3-llava-next-8b)")
    _materialise_derived_buffers(model)
    if adapter_path is not None:
        if not os.path.isdir(adapter_path):
            raise FileNotFoundError(f"load_llava: adapter directory {adapter_path!r} does not exist")
        try:
            from peft import PeftModel
            model = PeftModel.from_pretrained(model, adapter_path, device_map="cpu").merge_and_unload()
        except ImportError:
            merge_lora(model, adapter_path)
    model.eval().to(device=device, dtype=dtype)
    image_processor = CLIPImageProcessor.from_pretrained(config.mm_vision_tower)
    return tokenizer, model, image_processor


def _materialise_derived_buffers(model, force=False):
    """After a meta-device construction: re-create the buffers a checkpoint does not store (non-persistent ones) on the CPU.
    ``force``: re-create them even when they are not on the meta device (after ``to_empty`` they hold garbage)."""
    for mod in model.modules():
        for name, buf in list(mod._buffers.items()):
            if buf is None or not (buf.is_meta or (force and name in ("position_ids", "inv_freq", "original_inv_freq"))):
                continue
            if name == "position_ids":
                mod._buffers[name] = torch.arange(buf.shape[-1]).expand(buf.shape).clone()
            elif name in ("inv_freq", "original_inv_freq"):
                fn = getattr(mod, "rope_init_fn", None)
                if fn is not None:
                    inv, _ = fn(mod.config, "cpu")
                else:
                    base, dim = getattr(mod, "base", 10000.0), buf.shape[0] * 2
                    inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
                mod._buffers[name] = inv.to(torch.float32)
            else:
                raise RuntimeError(f"load_llava: buffer {name!r} of {type(mod).__name__} is neither in the checkpoint nor derivable")


def _eos_ids(model, tokenizer):
    ids = getattr(getattr(model, "generation_config", None), "eos_token_id", None)
    if ids is None:
        ids = getattr(model.config, "eos_token_id", None)
    if ids is None:
        ids = getattr(tokenizer, "eos_token_id", None)
    return [ids] if isinstance(ids, int) else list(ids or [])


def get_img_describe(image_tensor, image, model, tokenizer, prompt, conv_templates=conv_templates,
                     image_token_index=IMAGE_TOKEN_INDEX, conv_template="llava_llama_3", num_beams=1, temperature=0.2,
                     do_sample=True, max_new_tokens=512, device="cuda", seed=None, fast=None, decode_weights=None, decode_prefill=None,
                     decode_kernel=None, decode_attention=None):
    """models/util.py:17-66 -> ``[caption]``.  ``seed`` (an addition) makes the caption a function of (image, prompt,
    weights, seed): sampling then runs inside ``torch.random.fork_rng`` with the CPU and the model's device generator seeded
    THERE, so the caller's generators -- which Stage 2 draws its noise from right afterwards, and in the reference live on
    another device (infer.py:145-166: LLaVA on cuda:1) -- are exactly where they were, however many tokens were sampled.
    ``seed=None`` samples from the current generator state without touching any seed.
    ``fast`` (default: on a GPU, with one beam): the token loop runs through ``FastDecoder`` (static cache, decode step
    replayed from a hipGraph) instead of ``transformers``' ``generate``; same tokens (tests/test_llava_next.py).
    ``decode_weights`` (None = "native"): "e4m3" streams the token loop's weights as e4m3 bytes (``FastDecoder(weights=...)``, opt-in:
    other logits than the 16-bit weights give); "e4m3-only" runs the prefill on those bytes too and RELEASES the model's 16-bit decoder
    weights (``CAPTION_WEIGHTS``, ``caption_mode``: afterwards the model serves this mode only, until it is reloaded); both need the
    fast path, anything else raises.
    ``decode_prefill`` (None = "torch"): "flash" runs the prefill's attention through the causal flash kernel
    (``FastDecoder(prefill=...)``, opt-in: other logits than the torch prefill gives); it needs the fast path too.
    ``decode_kernel`` (None = "valu"): "mfma" runs the token loop's products on MFMAs (``FastDecoder(decode=...)``, ``CAPTION_DECODES``,
    opt-in: other logits, within the summation error); it needs the fast path too.
    ``decode_attention`` (None = "valu"): "mfma" runs the token loop's attention on MFMAs (``FastDecoder(decode_attention=...)``,
    ``CAPTION_ATTENTIONS``, opt-in: other logits); it needs the fast path too."""
    input_ids, mdev, fast, options = _describe_setup("get_img_describe", model, tokenizer, prompt, conv_templates, image_token_index, conv_template,
                                                     num_beams, device, fast, decode_weights, decode_prefill, decode_kernel, decode_attention)

    def run():
        if fast:   # (no_grad, not inference_mode: tensors made in inference mode cannot be updated in place by a later call
            with torch.no_grad():   # outside it, and a hipGraph capture that fails on that leaves the generator in capture state)
                return caption_tokens_fast(model, input_ids, image_tensor, [image.size], max_new_tokens, do_sample, temperature,
                                           _eos_ids(model, tokenizer), **options)
        with torch.inference_mode():
            return model.generate(input_ids, images=image_tensor, image_sizes=[image.size], do_sample=do_sample,
                                  temperature=temperature, num_beams=num_beams, max_new_tokens=max_new_tokens,
                                  return_dict_in_generate=True, output_scores=True)[0][0]

    if seed is None:
        out = run()
    else:
        with torch.random.fork_rng(devices=[mdev] if mdev.type == "cuda" else []):
            torch.manual_seed(seed)
            out = run()
    return [tokenizer.decode(out.cpu().tolist(), skip_special_tokens=True).lstrip()]


def _has_logits_warpers(model):
    """True when the checkpoint's generation_config asks for logits processing FastDecoder does not implement.  It implements what the
    reference's call uses: temperature, top_k (the config's value; transformers' default 50 IS applied by a sampling generate())
    and top_p; typical_p / min_p / penalties / banned or suppressed tokens are not."""
    g = getattr(model, "generation_config", None)
    if g is None:
        return False
    def differs(name, neutral):
        v = getattr(g, name, None)
        return v is not None and v != neutral
    return (differs("typical_p", 1.0) or differs("repetition_penalty", 1.0) or differs("no_repeat_ngram_size", 0)
            or differs("min_p", None) or differs("encoder_repetition_penalty", 1.0) or bool(getattr(g, "bad_words_ids", None))
            or bool(getattr(g, "suppress_tokens", None)))


def _describe_setup(who, model, tokenizer, prompt, conv_templates, image_token_index, conv_template, num_beams, device, fast, decode_weights,
                    decode_prefill, decode_kernel, decode_attention=None):
    """What ``get_img_describe`` and ``get_img_describe_batch`` (``who``) do before they caption: validate the four options and the
    template, tokenise the prompt, decide ``fast`` -> ``(input_ids, the model's device, fast, the options as caption_tokens_fast(_batch)
    keywords)``.  An option that is not its default needs the fast path and raises without it."""
    names = ("decode_weights", "decode_prefill", "decode_kernel", "decode_attention")
    options = dict(weights=decode_weights, prefill=decode_prefill, decode=decode_kernel, attention=decode_attention)
    default = caption_mode()
    mode = caption_mode(**options, who=who, names=names)
    if conv_template != "llava_llama_3":
        raise NotImplementedError("the pipeline's captioner is the Llama-3 LLaVA-NeXT (conv_template 'llava_llama_3')")
    system = getattr(conv_templates[conv_template], "system", LLAMA3_SYSTEM)
    text = llama3_prompt(tokenizer, prompt, system)
    input_ids = tokenizer_image_token(text, tokenizer, image_token_index, return_tensors="pt").unsqueeze(0).to(device)
    mdev = next(model.parameters()).device
    fast = (mdev.type == "cuda" and num_beams == 1) if fast is None else fast
    if fast and _has_logits_warpers(model):
        # FastDecoder implements generate()'s temperature / top_k / top_p chain; a generation_config with typical_p, min_p, penalties or
        # banned tokens goes through transformers' generate() (~4 x slower per token), and says so
        import warnings
        warnings.warn("llava_next: the checkpoint's generation_config asks for logits processors FastDecoder does not implement; "
                      "captioning through transformers' generate()")
        fast = False
    for name, field, value in zip(names, ("weights", "prefill", "decode", "decode_attention"), options.values()):
        if getattr(mode, field) != getattr(default, field) and not fast:
            raise ValueError(f"{who}: {name}={value!r} needs the FastDecoder token loop (a GPU model, one beam, no logits processors beyond "
                             f"temperature / top_k / top_p)")
    return input_ids, mdev, fast, options


def _decoder_for(model, need, rows, mode):
    """The model's ``FastDecoder`` (a plain attribute, ``model._fast_decoder``: not a submodule) for ``rows`` captions of ``need`` cache
    positions in ``mode``.  The one it has serves unless it is ``stale()`` -- the model was moved / cast / reloaded since the decoder
    fused its weights -- or in another mode, or holds fewer rows or a shorter cache; else it is dropped -- its cache, packs and captured
    graphs go before the new ones are allocated -- and one is built with ``rows`` rows and the cache length rounded up to 256."""
    dec = getattr(model, "_fast_decoder", None)
    if dec is None or dec.stale() or dec.mode != mode or dec.batch < rows or dec.max_len < need:
        model.__dict__.pop("_fast_decoder", None)
        del dec
        switches = dataclasses.asdict(mode)
        if mode.decode_attention == CaptionMode.decode_attention:      # (said only where it is asked for: a decoder class with the
            del switches["decode_attention"]                           # five-switch constructor goes on serving the default attention)
        model.__dict__["_fast_decoder"] = FastDecoder(model, -(-need // 256) * 256, batch=rows, **switches)
    return model._fast_decoder


def caption_tokens_fast(model, input_ids, images, image_sizes, max_new_tokens, do_sample, temperature, eos_ids=None, weights="native",
                        prefill="torch", decode="valu", attention="valu"):
    """Multimodal prompt -> generated token ids through the model's ``FastDecoder`` (built once per model, cache size, weight mode,
    prefill mode, decode kernel and decode attention: asking for another mode rebuilds the decoder, its packs and its captured graph; ``_decoder_for``).
    It goes on using a decoder with more rows than one."""
    mode = caption_mode(weights, prefill, decode, attention, who="caption_tokens_fast")
    embeds = model.multimodal_embeds(input_ids, images, image_sizes)
    dec = _decoder_for(model, embeds.shape[1] + max_new_tokens, 1, mode)
    return dec.generate(embeds, max_new_tokens, do_sample=do_sample, temperature=temperature, eos_token_id=eos_ids)


def caption_tokens_fast_batch(model, input_ids, images, image_sizes, max_new_tokens, do_sample, temperature, eos_ids=None, weights="native",
                              seeds=None, prefill="torch", decode="valu", attention="valu"):
    """``caption_tokens_fast`` for several images under ONE prompt: ``images[b]`` / ``image_sizes[b]`` are the views and the size of image
    ``b`` -> a list of token tensors, each equal to ``caption_tokens_fast`` on that image alone (under ``seeds[b]``, see
    ``FastDecoder.generate_batch``).  The model's decoder is rebuilt when it cannot hold this many rows, for another mode, or for a
    longer cache (``_decoder_for``).  The cache length is this
    group's longest prompt plus the new tokens, rounded up to 256 (kept if the decoder's is longer); the prefill runs over it, so the equality
    with the single call holds where both prefill the image at the same cache length (the decode step does not depend on it) -- or, with
    ``prefill="flash"``, at any cache length: that prefill does not depend on it either.  ``decode``, ``attention``: as in ``caption_tokens_fast``."""
    mode = caption_mode(weights, prefill, decode, attention, who="caption_tokens_fast_batch")
    embeds = [model.multimodal_embeds(input_ids, im, [size]) for im, size in zip(images, image_sizes)]
    dec = _decoder_for(model, max(e.shape[1] for e in embeds) + max_new_tokens, len(embeds), mode)
    return dec.generate_batch(embeds, max_new_tokens, do_sample=do_sample, temperature=temperature, eos_token_id=eos_ids, seeds=seeds)


def get_img_describe_batch(image_tensors, images, model, tokenizer, prompt, conv_templates=conv_templates,
                           image_token_index=IMAGE_TOKEN_INDEX, conv_template="llava_llama_3", num_beams=1, temperature=0.2,
                           do_sample=True, max_new_tokens=512, device="cuda", seeds=None, fast=None, decode_weights=None, decode_prefill=None,
                           decode_kernel=None, decode_attention=None):
    """``get_img_describe`` for a list of images (``image_tensors[b]``: the views of ``images[b]``) under one prompt -> a list of captions,
    caption ``b`` being what ``get_img_describe(image_tensors[b], images[b], ..., seed=seeds[b])[0]`` returns: with the FastDecoder the
    token loops of all images run as one (the decoder's weights are streamed once per step for all of them); without it the images
    are captioned one after another.  ``seeds``: one seed per image, or None (sample from the current generator state)."""
    n = len(images)
    if len(image_tensors) != n or (seeds is not None and len(seeds) != n):
        raise ValueError(f"get_img_describe_batch: {len(image_tensors)} view lists and {None if seeds is None else len(seeds)} seeds for {n} images")
    input_ids, _, use_fast, options = _describe_setup("get_img_describe_batch", model, tokenizer, prompt, conv_templates, image_token_index,
                                                      conv_template, num_beams, device, fast, decode_weights, decode_prefill, decode_kernel,
                                                      decode_attention)
    if not use_fast or n > FastDecoder.MAX_BATCH:
        return [get_img_describe(image_tensors[b], images[b], model, tokenizer, prompt, conv_templates, image_token_index, conv_template,
                                 num_beams, temperature, do_sample, max_new_tokens, device, None if seeds is None else seeds[b], use_fast,
                                 decode_weights, decode_prefill, decode_kernel, decode_attention)[0] for b in range(n)]
    with torch.no_grad():
        outs = caption_tokens_fast_batch(model, input_ids, image_tensors, [im.size for im in images], max_new_tokens, do_sample, temperature,
                                         _eos_ids(model, tokenizer), seeds=seeds, **options)
    return [tokenizer.decode(o.cpu().tolist(), skip_special_tokens=True).lstrip() for o in outs]
