"""``FastDecoder(weights="e4m3", prefill_weights="e4m3")`` and ``release_native=True`` on the GPU, on the seeded 3-layer Llama of
tests/test_gpu_w8.py and its dequantised twin, behind a 300-token prompt: the caption is ONE model, prefill included; with the flash
prefill nothing depends on the cache length or on the batch; the 16-bit weights really go, within the stated memory bounds, and the
model left behind serves this mode only.  Every test here passes ``prefill_weights`` and so fails on a tree without the keyword."""
import copy
import gc

import pytest
import torch

from test_gpu_w8 import _dequantised_copy, _seeded_llama

pytestmark = pytest.mark.gpu

ROUTES = ["torch", "flash"]
ONLY = dict(weights="e4m3", prefill_weights="e4m3")


def _prompt(cfg, cuda, n=300, seed=3):
    return torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(seed)).to(cuda)


def _teacher_forced(dec, emb, toks):
    """test_gpu_w8's helper with ``pos0`` (the flash prefill asks for it): prefill, then one eager decode step per token of ``toks``
    -> logits ``[1 + len(toks), vocab]`` (fp32, on the host)."""
    T0 = emb.shape[1]
    embed = dec.model.model.embed_tokens
    with torch.no_grad():
        out = [dec.forward(emb.to(dec.dt), torch.arange(T0, device=dec.dev), pos0=0).float().cpu()]
        for n, tok in enumerate(toks):
            out.append(dec.forward(embed(tok.view(1))[None], torch.tensor([T0 + n], device=dec.dev)).float().cpu())
    return torch.cat(out)


def _projections(model):
    mods = []
    for layer in model.model.layers:
        at, mlp = layer.self_attn, layer.mlp
        mods += [at.q_proj, at.k_proj, at.v_proj, at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj]
    return mods


@pytest.mark.parametrize("route", ROUTES)
def test_one_model_prefill_included(cuda, route):
    """On the dequantised twin the e4m3-only decoder and the native one multiply the SAME numbers from the first prompt token on: prefill
    logits and 23 teacher-forced decode logits agree within the bound test_fast_decoder_e4m3_token_loop uses for this pair of decoders
    (summation order only).  On the ORIGINAL model the e4m3 prefill is another model than the 16-bit prefill of ``weights="e4m3"``."""
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda)
    twin = _dequantised_copy(model)
    emb = twin.model.embed_tokens(_prompt(cfg, cuda))
    dec_p = LN.FastDecoder(twin, 400, prefill=route, **ONLY)
    assert (dec_p.weights, dec_p.prefill_weights, dec_p.release_native) == ("e4m3", "e4m3", False)
    with torch.no_grad():
        toks = dec_p.generate(emb, 24, do_sample=False)
    lp = _teacher_forced(LN.FastDecoder(twin, 400, prefill=route, **ONLY), emb, toks[:-1])
    ln = _teacher_forced(LN.FastDecoder(twin, 400, prefill=route), emb, toks[:-1])
    assert lp.argmax(-1).tolist() == toks.cpu().tolist()
    for n in range(24):
        d, rng = float((lp[n] - ln[n]).abs().max()), float(ln[n].abs().max())
        print(f"{route} {'prefill' if n == 0 else f'step {n}'}: e4m3-only vs native on dequantised weights, logits max|d| = {d:.3e} (range {rng:.2f})")
        assert d < 2e-2 * rng, (n, d, rng)
    # nothing was mutated: the twin's weights are still what they were
    assert all(m.weight.numel() > 0 for m in _projections(twin)) and LN.FastDecoder.PARKED not in twin.__dict__
    emb_o = model.model.embed_tokens(_prompt(cfg, cuda))
    T0 = emb_o.shape[1]
    with torch.no_grad():
        l8 = LN.FastDecoder(model, 400, prefill=route, **ONLY).forward(emb_o, torch.arange(T0, device=cuda), pos0=0)
        l16 = LN.FastDecoder(model, 400, prefill=route, weights="e4m3").forward(emb_o, torch.arange(T0, device=cuda), pos0=0)
    assert bool(torch.isfinite(l8).all()) and not torch.equal(l8, l16), "the prefill still runs on the 16-bit weights"


def test_nothing_depends_on_the_cache_length_or_the_batch(cuda):
    """``prefill="flash"`` + ``prefill_weights="e4m3"``: every operator of the prefill is row-invariant, so prefill logits, the written
    cache rows and 24 greedy tokens are equal at ``max_len`` 512 and 768, and ``generate_batch`` of three prompts equals three
    ``generate`` runs, greedy and sampled."""
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda)
    embed = model.model.embed_tokens
    emb = embed(_prompt(cfg, cuda))
    T0 = emb.shape[1]
    res = []
    for max_len in (512, 768):
        dec = LN.FastDecoder(model, max_len, prefill="flash", **ONLY)
        with torch.no_grad():
            logits = dec.forward(emb, torch.arange(T0, device=cuda), pos0=0).clone()
            rows = [t[0][:, :T0].clone() for t in dec.k + dec.v]
            toks = dec.generate(emb, 24, do_sample=False)
        res.append((logits, rows, toks))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert torch.equal(res[0][2], res[1][2]) and len(res[0][2]) == 24
    prompts = [embed(_prompt(cfg, cuda, n, seed)) for n, seed in ((300, 3), (150, 4), (40, 5))]
    seeds = [11, 12, 13]
    dec = LN.FastDecoder(model, 512, batch=3, prefill="flash", **ONLY)
    for sample in (False, True):
        kw = dict(do_sample=sample, temperature=0.7)
        with torch.no_grad():
            single = []
            for e, s in zip(prompts, seeds):
                with torch.random.fork_rng(devices=[cuda]):
                    torch.manual_seed(s)
                    single.append(dec.generate(e, 8, **kw))
            together = dec.generate_batch(prompts, 8, seeds=seeds, **kw)
        assert [t.tolist() for t in together] == [t.tolist() for t in single], sample


def _nbytes(t):
    return t.numel() * t.element_size()


_measured = {}


def _release_measured(cuda):
    """ONE release on a fresh seeded model from an empty allocator cache (nothing but the model and what the constructor makes is in
    the allocator's lists), with ``torch.cuda.memory_allocated`` before and after and the peak in between -- shared by the two memory tests."""
    if not _measured:
        from rsvld_amd import llava_next as LN
        model, cfg = _seeded_llama(cuda)
        released = _projections(model) + [model.lm_head]
        m = dict(layer_src=sum(_nbytes(x.weight) for x in _projections(model)[:7]), released=sum(_nbytes(x.weight) for x in released))
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        m["base"], m["base_requested"] = torch.cuda.memory_allocated(), torch.cuda.memory_stats().get("requested_bytes.all.current")
        torch.cuda.reset_peak_memory_stats()
        dec = LN.FastDecoder(model, 512, prefill="flash", release_native=True, **ONLY)
        torch.cuda.synchronize()
        m["after"], m["peak"] = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
        m["after_requested"] = torch.cuda.memory_stats().get("requested_bytes.all.current")      # (printed beside the figure the test is about)
        flat = [p for layer in dec._packs[:-1] for p in layer] + [dec._packs[-1]]
        m["packs"] = sum(_nbytes(q) + _nbytes(s) for q, s in flat)
        m["layer_packs"] = sum(_nbytes(q) + _nbytes(s) for q, s in dec._packs[0])
        m["caches"] = sum(_nbytes(t) for t in dec.k + dec.v) + _nbytes(dec.cols)
        assert dec._ws_rows is None                                   # the decode workspace comes with the first step: 0 bytes here
        assert all(x.weight.numel() == 0 for x in released)
        m["slack"] = 512 * (2 * len(flat) + len(dec.k) + len(dec.v) + 1 + len(released))      # 512 B per tensor involved
        print("release:", m)
        _measured.update(m)
    return _measured


def test_release_native_resident_memory(cuda):
    """``memory_allocated`` with the released decoder built is at most its value before + packs + caches (+ no workspace yet) - the
    released bytes, 512 B of allocator rounding allowed per tensor involved.

    torch's caching allocator does not split a large block when 1 MiB or less would remain, and this model's tensors are 0.5-4 MiB: a
    pack that takes the slightly larger hole a released source left is accounted with the whole hole.  ``FastDecoder._pack_tight`` puts
    every pack into a block of its own size; without it this figure stood 2 167 488 bytes above the bound (alone) and 21 184 (behind the
    rest of the suite), with it 960 bytes above the bytes REQUESTED from the allocator, which are printed beside it."""
    m = _release_measured(cuda)
    assert m["after"] <= m["base"] + m["packs"] + m["caches"] - m["released"] + m["slack"], m


def test_release_native_peak_memory(cuda):
    """While it is built, allocated memory never stands more than one layer's sources above the packs and caches made so far: the packs of
    the layers before are smaller than what those layers released, so the first layer is the high-water mark."""
    m = _release_measured(cuda)
    assert m["peak"] <= m["base"] + m["caches"] + m["layer_packs"] + m["layer_src"] + m["slack"], m


@pytest.mark.parametrize("route", ROUTES)
def test_release_native(cuda, route):
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda)
    model.model.mm_projector = torch.nn.Linear(16, 16).to(cuda, torch.float16)        # a stand-in for the vision side
    ref = copy.deepcopy(model)
    emb = ref.model.embed_tokens(_prompt(cfg, cuda))
    T0 = emb.shape[1]
    dec_ref = LN.FastDecoder(ref, 512, prefill=route, **ONLY)
    with torch.no_grad():
        want_logits = dec_ref.forward(emb, torch.arange(T0, device=cuda), pos0=0).clone()
        want_toks = dec_ref.generate(emb, 24, do_sample=False)
        want_last = dec_ref._logits.clone()
    del dec_ref
    released = _projections(model) + [model.lm_head]
    dec = LN.FastDecoder(model, 512, prefill=route, release_native=True, **ONLY)
    assert all(m.weight.numel() == 0 and m.weight.dtype == torch.float16 and m.weight.device == cuda for m in released)
    assert model.__dict__[LN.FastDecoder.PARKED] is dec._packs and dec.release_native
    for name in ("model.embed_tokens.weight", "model.norm.weight", "model.mm_projector.weight", "model.layers.0.input_layernorm.weight",
                 "model.layers.2.post_attention_layernorm.weight"):
        assert torch.equal(model.get_parameter(name), ref.get_parameter(name)), name
    with torch.no_grad():
        assert torch.equal(dec.forward(emb, torch.arange(T0, device=cuda), pos0=0), want_logits)
        assert torch.equal(dec.generate(emb, 24, do_sample=False), want_toks) and torch.equal(dec._logits, want_last)
        # a longer cache: the packs are adopted (their sources no longer exist), same logits -- bit for bit with the flash prefill; the
        # torch prefill itself runs over the whole cache and promises no bits across cache lengths: the decoders' bound
        dec2 = LN.FastDecoder(model, 768, prefill=route, **ONLY)
        assert dec2._packs is dec._packs and dec2.release_native and not dec2.stale()
        got = dec2.forward(emb, torch.arange(T0, device=cuda), pos0=0)
        if route == "flash":
            assert torch.equal(got, want_logits)
        else:
            assert float((got.float() - want_logits.float()).abs().max()) < 2e-2 * float(want_logits.float().abs().max())
    for kw in (dict(), dict(weights="e4m3"), dict(prefill="flash")):
        with pytest.raises(RuntimeError, match="reload the model"):
            LN.FastDecoder(model, 512, **kw)
    with pytest.raises(RuntimeError, match="reload the model"):
        LN.merge_lora(model, "unused")
    assert not dec.stale()
    up = model.model.layers[1].mlp.up_proj
    up.weight.data = torch.zeros(cfg.intermediate_size, cfg.hidden_size, device=cuda, dtype=torch.float16)
    assert dec.stale() and dec2.stale()
    with pytest.raises(RuntimeError, match="reload the model"):      # ... and such a model's packs are not adopted either
        LN.FastDecoder(model, 512, prefill=route, **ONLY)


def test_release_keeps_a_tied_head(cuda):
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda, layers=1)
    model.lm_head.weight = model.model.embed_tokens.weight
    table = model.model.embed_tokens.weight.clone()
    dec = LN.FastDecoder(model, 256, release_native=True, **ONLY)
    assert all(m.weight.numel() == 0 for m in _projections(model))
    assert model.lm_head.weight is model.model.embed_tokens.weight and torch.equal(model.lm_head.weight, table)
    assert not dec.stale()
    emb = model.model.embed_tokens(_prompt(cfg, cuda, 20))
    with torch.no_grad():
        assert len(dec.generate(emb, 4, do_sample=False)) == 4
    assert not LN.FastDecoder(model, 512, **ONLY).stale()            # adopted, the head still tied


@pytest.mark.parametrize("route", ROUTES)
def test_caption_tokens_fast_e4m3_only(cuda, route):
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda, layers=1)
    model.multimodal_embeds = lambda ids, images, sizes: model.model.embed_tokens(ids)
    ids = _prompt(cfg, cuda, 20, 4)
    run = lambda mode, n=4: LN.caption_tokens_fast(model, ids, None, None, n, False, 1.0, None, weights=mode, prefill=route)
    with torch.no_grad():
        a = run("e4m3-only")
        d0 = model._fast_decoder
        assert (d0.weights, d0.prefill_weights, d0.release_native) == ("e4m3", "e4m3", True) and d0._graph is not None
        assert all(m.weight.numel() == 0 for m in _projections(model) + [model.lm_head])
        assert torch.equal(run("e4m3-only"), a) and model._fast_decoder is d0
        b = run("e4m3-only", 300)                                     # a longer cache: rebuilt on the parked packs
        d1 = model._fast_decoder
        assert d1 is not d0 and d1.max_len > d0.max_len and d1._packs is d0._packs and len(b) == 300
        assert route != "flash" or torch.equal(b[:4], a)              # (the torch prefill depends on the cache length by itself)
        outs = LN.caption_tokens_fast_batch(model, ids, [None, None], [None, None], 4, False, 1.0, None, weights="e4m3-only", prefill=route)
        d2 = model._fast_decoder                                      # two rows: rebuilt again, at the first call's cache length
        assert d2.batch == 2 and d2._packs is d0._packs and d2.max_len == d0.max_len
        assert all(torch.equal(o, a) for o in outs)
        for mode in ("native", "e4m3"):
            with pytest.raises(RuntimeError, match="reload the model"):
                run(mode)
