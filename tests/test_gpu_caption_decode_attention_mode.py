"""``FastDecoder(decode_attention="mfma")``: the token loop's attention on MFMAs (dam_kernel of csrc/decode_attention.hip).  Inside the mode a
batched caption is the one-at-a-time caption token for token (a sequence's bits do not depend on the row count: ``generate``'s single
row runs the MFMA attention too), with 16-bit and e4m3 weights and with the products on either family of kernels; against the default
attention the logits move by the rounding of P where the scores used to be rounded -- within the token loop's own tolerance, 2e-2 x the
logit range; the launches are those tests/test_gpu_caption_launch_sequence.py pins with the attention's name exchanged, and the default
launches what it launched."""
import pytest
import torch

from test_gpu_caption_decode_mfma import _lists, _singles
from test_gpu_caption_e4m3_only import _teacher_forced
from test_gpu_caption_launch_sequence import MODES, record
from test_gpu_decode_rows import MAX_LEN, NEW, PROMPTS
from test_gpu_w8 import _seeded_llama

pytestmark = pytest.mark.gpu

VALU, MMA = "llama_decode_attention_rows", "llama_decode_attention_mma_rows"


@pytest.fixture(scope="module")
def llama(cuda):
    model, cfg = _seeded_llama(cuda, layers=2)
    embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(cuda))
            .detach() for n in PROMPTS]
    return model, embs


@pytest.mark.parametrize("decode", ["valu", "mfma"])
@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_generate_batch_equals_three_generate_runs_in_the_mode(cuda, llama, weights, decode):
    """Greedy, sampled (temperature 0.7, seeds 1 / 2 / 3) and an early end token, through the captured graph; greedy eagerly too."""
    import guarded
    from rsvld_amd import llava_next as LN, ops
    model, embs = llama
    seeds = [1, 2, 3]
    kw = dict(weights=weights, decode=decode, decode_attention="mfma")
    dec1 = LN.FastDecoder(model, MAX_LEN, **kw)
    assert dec1.decode_attention == "mfma" and dec1.mode.decode_attention == "mfma"
    greedy, sampled, eos, ended = _singles(dec1, embs, cuda, seeds)
    rec = guarded.LaunchRecorder()
    with ops.tuning(profiler=rec):                              # the single row ran the MFMA attention, and no VALU one
        dec1.generate(embs[0], 3, do_sample=False, use_graph=False)
    assert rec.ran(MMA) and not rec.ran(VALU), rec.names
    del dec1
    decb = LN.FastDecoder(model, MAX_LEN, batch=3, **kw)
    assert _lists(decb.generate_batch(embs, NEW, do_sample=False)) == _lists(greedy)
    assert _lists(decb.generate_batch(embs, NEW, do_sample=True, temperature=0.7, seeds=seeds)) == _lists(sampled)
    assert _lists(decb.generate_batch(embs, NEW, do_sample=False, eos_token_id=eos)) == _lists(ended)
    assert _lists(decb.generate_batch(embs, NEW, do_sample=False, use_graph=False)) == _lists(greedy)


@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_distance_from_the_default_attention(cuda, llama, weights):
    """The prefill is shared; 23 teacher-forced decode steps against the ``decode_attention="valu"`` decoder on the same weights."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    emb = embs[2]
    toks = LN.FastDecoder(model, MAX_LEN, weights=weights).generate(emb, NEW, do_sample=False)
    lv = _teacher_forced(LN.FastDecoder(model, MAX_LEN, weights=weights), emb, toks[:-1])
    lm = _teacher_forced(LN.FastDecoder(model, MAX_LEN, weights=weights, decode_attention="mfma"), emb, toks[:-1])
    assert torch.equal(lv[0], lm[0]), "the prefill is not part of the mode"
    assert NEW - 1 == 23
    worst = 0.0
    for n in range(1, NEW):
        d, rng = float((lm[n] - lv[n]).abs().max()), float(lv[n].abs().max())
        worst = max(worst, d / rng)
        print(f"step {n}: logits max|d| / range = {d / rng:.3e}")
    print(f"decode_attention=mfma vs valu, {weights} weights, 23 teacher-forced steps: worst logits max|d| / range = {worst:.3e} (bound 2e-2)")
    assert worst < 2e-2, worst


@pytest.mark.parametrize("name", list(MODES))
def test_launch_sequence_with_the_attention_exchanged(cuda, name):
    mode, build, prefill, step = MODES[name]
    step = [MMA if s == VALU else s for s in step]
    assert step.count(MMA) == 2 and VALU not in step
    got_build, got_one, got_rows = record(dict(mode, decode_attention="mfma"), 2, cuda)
    assert got_build == build and got_one == prefill + step and got_rows == prefill + prefill + step


def test_the_default_attention_launches_what_it_launched(cuda):
    mode, build, prefill, step = MODES["mfma"]
    got_build, got_one, got_rows = record(dict(mode, decode_attention="valu"), 2, cuda)
    assert got_build == build and got_one == prefill + step and got_rows == prefill + prefill + step


def test_the_mode_needs_the_fused_step_and_never_falls_back(cuda, llama):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    dec = LN.FastDecoder(model, MAX_LEN, batch=2, decode_attention="mfma")
    dec.fused = False                                           # ``_fused_ok`` fails
    with pytest.raises(RuntimeError, match="decode_attention='mfma'"):
        dec.generate(embs[0], 4, do_sample=False, use_graph=False)
    with pytest.raises(RuntimeError, match="decode_attention='mfma'"):
        dec.generate_batch(embs[:2], 4, do_sample=False)


def test_decoder_for_rebuilds_when_only_this_field_differs(cuda, llama, monkeypatch):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    monkeypatch.setattr(model, "multimodal_embeds", lambda ids, im, sizes: embs[0], raising=False)
    model.__dict__.pop("_fast_decoder", None)
    try:
        LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, decode="mfma")
        first = model._fast_decoder
        assert first.decode_attention == "valu" and first.decode == "mfma"
        b = LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, decode="mfma", attention="mfma")
        second = model._fast_decoder
        assert second is not first and second.decode_attention == "mfma" and second.decode == "mfma"
        outs = LN.caption_tokens_fast_batch(model, None, [None], [None], 4, False, 1.0, decode="mfma", attention="mfma")
        assert model._fast_decoder is second and outs[0].tolist() == b.tolist()
        LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, decode="mfma")
        assert model._fast_decoder is not second and model._fast_decoder.decode_attention == "valu"
        with pytest.raises(ValueError, match="attention"):
            LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, attention="x")
    finally:
        model.__dict__.pop("_fast_decoder", None)
