"""``FastDecoder(decode="mfma")``: the token loop on the MFMA products (csrc/gemv_mma.hip).  Inside the mode a batched caption is the
one-at-a-time caption token for token (a row's bits do not depend on the row count: ``generate``'s single row runs the MFMA kernels
too); against the default mode the logits move by the order of an fp32 sum -- within the tolerance tests/test_gpu_caption_e4m3_only.py
uses for the token loop, 2e-2 x the logit range."""
import pytest
import torch

from test_gpu_caption_e4m3_only import _teacher_forced
from test_gpu_decode_rows import MAX_LEN, NEW, PROMPTS
from test_gpu_w8 import _seeded_llama

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def llama(cuda):
    model, cfg = _seeded_llama(cuda, layers=2)
    embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(cuda))
            .detach() for n in PROMPTS]
    return model, embs


def _singles(dec1, embs, cuda, seeds):
    greedy = [dec1.generate(e, NEW, do_sample=False) for e in embs]
    sampled = []
    for e, s in zip(embs, seeds):
        with torch.random.fork_rng(devices=[cuda]):
            torch.manual_seed(s)
            sampled.append(dec1.generate(e, NEW, do_sample=True, temperature=0.7))
    eos = int(greedy[1][4])                                     # row 1 ends around its fifth token
    ended = [dec1.generate(e, NEW, do_sample=False, eos_token_id=eos) for e in embs]
    assert len(ended[1]) <= 5 and int(ended[1][-1]) == eos and all(len(t) == NEW for t in greedy + sampled)
    assert any(len(t) > len(ended[1]) for t in ended), "every row ends as early as row 1: the case shows nothing"
    return greedy, sampled, eos, ended


def _lists(ts):
    return [t.tolist() for t in ts]


@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_generate_batch_equals_three_generate_runs_in_the_mode(cuda, llama, weights):
    """Greedy, sampled (temperature 0.7, seeds 1 / 2 / 3) and an early end token; through the captured graph and eagerly; then fewer
    prompts than rows."""
    from rsvld_amd import llava_next as LN
    import guarded
    from rsvld_amd import ops
    model, embs = llama
    seeds = [1, 2, 3]
    dec1 = LN.FastDecoder(model, MAX_LEN, weights=weights, decode="mfma")
    assert dec1.decode == "mfma"
    greedy, sampled, eos, ended = _singles(dec1, embs, cuda, seeds)
    rec = guarded.LaunchRecorder()
    with ops.tuning(profiler=rec):                              # the single row ran the MFMA kernels, and no VALU product
        dec1.generate(embs[0], 3, do_sample=False, use_graph=False)
    mma, valu = ("gemv_w8_mma_rows", "gemv_w8_rows") if weights == "e4m3" else ("gemv_mma_rows", "gemv_rows")
    assert rec.ran(mma) and not rec.ran(valu), rec.names
    del dec1

    decb = LN.FastDecoder(model, MAX_LEN, weights=weights, batch=3, decode="mfma")
    for use_graph in (True, False):
        assert _lists(decb.generate_batch(embs, NEW, do_sample=False, use_graph=use_graph)) == _lists(greedy), ("greedy", use_graph)
        got = decb.generate_batch(embs, NEW, do_sample=True, temperature=0.7, seeds=seeds, use_graph=use_graph)
        assert _lists(got) == _lists(sampled), ("sampled", use_graph)
        got = decb.generate_batch(embs, NEW, do_sample=False, eos_token_id=eos, use_graph=use_graph)
        assert _lists(got) == _lists(ended), ("eos", use_graph)
    two = decb.generate_batch(embs[1:], NEW, do_sample=False)   # fewer prompts than rows
    assert _lists(two) == _lists(greedy[1:])


def test_the_mode_combines_with_flash_prefill_and_released_weights(cuda):
    """``prefill="flash"``, ``prefill_weights="e4m3"``, ``release_native=True`` on a model of its own (its 16-bit weights go)."""
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda, layers=2)
    embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(cuda))
            .detach() for n in PROMPTS]
    kw = dict(weights="e4m3", prefill="flash", prefill_weights="e4m3", release_native=True, decode="mfma")
    dec1 = LN.FastDecoder(model, MAX_LEN, **kw)
    greedy = [dec1.generate(e, NEW, do_sample=False) for e in embs]
    del dec1
    decb = LN.FastDecoder(model, MAX_LEN, batch=3, **kw)        # adopts the parked packs
    assert decb.release_native and decb.decode == "mfma"
    assert _lists(decb.generate_batch(embs, NEW, do_sample=False)) == _lists(greedy)


@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_distance_from_the_default_mode(cuda, llama, weights):
    """The prefill is shared (untouched by the mode); 23 teacher-forced decode steps: the logits of ``decode="mfma"`` against
    ``decode="valu"`` on the same weights, within 2e-2 x the logit range (the token loop's tolerance in test_gpu_caption_e4m3_only.py).
    Measured: see profiles/caption_decode_mfma_ab.txt."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    emb = embs[2]
    toks = LN.FastDecoder(model, MAX_LEN, weights=weights).generate(emb, NEW, do_sample=False)
    lv = _teacher_forced(LN.FastDecoder(model, MAX_LEN, weights=weights), emb, toks[:-1])
    lm = _teacher_forced(LN.FastDecoder(model, MAX_LEN, weights=weights, decode="mfma"), emb, toks[:-1])
    assert torch.equal(lv[0], lm[0]), "the prefill is not part of the mode"
    worst = 0.0
    for n in range(1, NEW):
        d, rng = float((lm[n] - lv[n]).abs().max()), float(lv[n].abs().max())
        worst = max(worst, d / rng)
        assert d < 2e-2 * rng, (n, d, rng)
    print(f"decode=mfma vs valu, {weights} weights, 23 teacher-forced steps: worst logits max|d| / range = {worst:.3e} (bound 2e-2)")


def test_the_mode_needs_the_fused_step_and_never_falls_back(cuda, llama):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    dec = LN.FastDecoder(model, MAX_LEN, batch=2, decode="mfma")
    dec.fused = False                                           # ``_fused_ok`` fails
    with pytest.raises(RuntimeError, match="mfma"):
        dec.generate(embs[0], 4, do_sample=False, use_graph=False)
    with pytest.raises(RuntimeError, match="mfma"):
        dec.generate_batch(embs[:2], 4, do_sample=False)


def test_caption_tokens_fast_rebuilds_the_decoder_for_the_mode(cuda, llama, monkeypatch):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    monkeypatch.setattr(model, "multimodal_embeds", lambda ids, im, sizes: embs[0], raising=False)
    model.__dict__.pop("_fast_decoder", None)
    try:
        a = LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0)
        first = model._fast_decoder
        assert first.decode == "valu"
        LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0)
        assert model._fast_decoder is first
        b = LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, decode="mfma")
        assert model._fast_decoder is not first and model._fast_decoder.decode == "mfma"
        second = model._fast_decoder
        outs = LN.caption_tokens_fast_batch(model, None, [None], [None], 4, False, 1.0, decode="mfma")
        assert model._fast_decoder is second and outs[0].tolist() == b.tolist()
        LN.caption_tokens_fast_batch(model, None, [None], [None], 4, False, 1.0)
        assert model._fast_decoder.decode == "valu"
        assert len(a) == len(b) == 4
        with pytest.raises(ValueError, match="decode"):
            LN.caption_tokens_fast(model, None, None, None, 4, False, 1.0, decode="x")
    finally:
        model.__dict__.pop("_fast_decoder", None)
