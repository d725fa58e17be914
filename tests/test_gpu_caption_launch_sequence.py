"""The launches of one caption prefill plus one decode step, by name and in order, in every ``FastDecoder`` mode.

Host-side changes to ``llava_next.FastDecoder`` (how it holds its weights, how it picks a product's kernel) must leave every launch, and
the order of the launches, what they are: this test pins them.  ``ops.LaunchProfiler`` under ``ops.tuning(profiler=...)`` records the
name of every launch of the library; the decoder runs eagerly (``use_graph=False``: a replayed graph launches nothing from the host).
The model is the seeded Llama of tests/test_gpu_w8.py (head_dim 128) with two layers, the prompts are 5 (and 3) tokens long, and two new
tokens are asked for: the prefill, which also gives the first token, and ONE decode step.  What torch launches itself (RMSNorm, rotary
embedding and the attention of the torch prefill, sampling) does not pass through the library and is not recorded."""
import pytest
import torch

from test_gpu_w8 import _seeded_llama

pytestmark = pytest.mark.gpu

LAYERS = 2
ALL = dict(weights="e4m3", prefill="flash", prefill_weights="e4m3", release_native=True, decode="mfma")

# ---- what ONE layer launches (q|k|v, [attention], o_proj, gate|up, down_proj), then the head
# the prefill of T > 1 rows: 16-bit weights go through torch (F.linear, not recorded); the head's single row is the library's GEMV
PREFILL_TORCH = ["gemv"]
PREFILL_FLASH = ["llama_prefill_attention"] * LAYERS + ["gemv"]
PREFILL_W8_FLASH = ["linear_w8", "llama_prefill_attention", "linear_w8", "linear_w8", "linear_w8"] * LAYERS + ["gemv_w8"]
# the fused decode step: four products and one attention per layer, then norm + lm_head
STEP = {
    "valu": ["gemv_rows", "llama_decode_attention_rows", "gemv_rows", "gemv_rows", "gemv_rows"] * LAYERS + ["gemv_rows"],
    "valu_w8": ["gemv_w8_rows", "llama_decode_attention_rows", "gemv_w8_rows", "gemv_w8_rows", "gemv_w8_rows"] * LAYERS + ["gemv_w8_rows"],
    "mfma": ["gemv_mma_rows", "llama_decode_attention_rows", "gemv_mma_rows", "gemv_mma_rows", "gemv_mma_rows"] * LAYERS + ["gemv_mma_rows"],
    "mfma_w8": ["gemv_w8_mma_rows", "llama_decode_attention_rows", "gemv_w8_mma_rows", "gemv_w8_mma_rows", "gemv_w8_mma_rows"] * LAYERS
               + ["gemv_w8_mma_rows"],
}
PACK = ["pack_rows_e4m3"] * (4 * LAYERS + 1)      # building an e4m3 decoder: four packs per layer, then lm_head's

# mode -> (keywords, launches of the constructor, of one prompt's prefill, of the decode step)
MODES = {
    "default": ({}, [], PREFILL_TORCH, STEP["valu"]),
    "e4m3": (dict(weights="e4m3"), PACK, PREFILL_TORCH, STEP["valu_w8"]),
    "flash": (dict(prefill="flash"), [], PREFILL_FLASH, STEP["valu"]),
    "mfma": (dict(decode="mfma"), [], PREFILL_TORCH, STEP["mfma"]),
    "all": (ALL, PACK, PREFILL_W8_FLASH, STEP["mfma_w8"]),
}


def record(mode, batch, cuda):
    """-> (launch names of ``FastDecoder(**mode)``'s construction, of ``generate`` on a 5-token prompt, of ``generate_batch`` on prompts
    of 5 and 3 tokens), two new tokens each, on a model of its own (a released model serves no other mode)."""
    from rsvld_amd import llava_next as LN, ops
    model, cfg = _seeded_llama(cuda, layers=LAYERS)
    ids = torch.randint(0, cfg.vocab_size, (1, 5), generator=torch.Generator().manual_seed(5)).to(cuda)
    emb = model.model.embed_tokens(ids)
    out = []
    with torch.no_grad():
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            dec = LN.FastDecoder(model, 256, batch=batch, **mode)
        out.append([r[0] for r in prof.records])
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            toks = dec.generate(emb, 2, do_sample=False, use_graph=False)
        out.append([r[0] for r in prof.records])
        with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
            rows = dec.generate_batch([emb, emb[:, :3]], 2, do_sample=False, use_graph=False)
        out.append([r[0] for r in prof.records])
    assert len(toks) == 2 and [len(r) for r in rows] == [2, 2] and dec._graph is None and not dec._rows
    return out


@pytest.mark.parametrize("name", list(MODES))
def test_caption_launch_sequence(cuda, name):
    mode, build, prefill, step = MODES[name]
    got_build, got_one, got_rows = record(mode, 2, cuda)
    print(f"{name}: build {got_build}\n{name}: generate {got_one}\n{name}: generate_batch {got_rows}")
    assert got_build == build
    assert got_one == prefill + step                   # one prompt: its prefill, then one step
    assert got_rows == prefill + prefill + step        # two prompts: prefill after prefill, then ONE step for both rows
