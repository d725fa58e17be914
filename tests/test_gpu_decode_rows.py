"""The multi-row decode operators (rsvld_amd/decode_rows.py) and the batched token loop (``FastDecoder.generate_batch``) against their
single-row siblings.  The contract is bit-identity per row, so every comparison is ``torch.equal``: no tolerance anywhere in this file."""
import pytest
import torch

from test_gpu_w8 import _seeded_llama

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}
ROWS = (1, 2, 3, 5, 8)
# (N, K).  16-bit weights: row route with an odd step + an 8-element tail and rows past N; K-split route with and without the two-step
# loop; K-split route whose eight staged rows exceed the LDS (walked in two groups)
NATIVE_SHAPES = [(37, 1544), (20, 2048), (20, 4096), (24, 14336)]
# e4m3: one piece; row route, ragged; K-split route a quarter shorter than one step; K-split route, 3.5 steps per quarter
W8_SHAPES = [(17, 16), (37, 1552), (20, 3584), (24, 14336)]


def _operands(cuda, N, K, dtype):
    g = torch.Generator().manual_seed(1000 * N + K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dtype)
    x = torch.randn(8, K, generator=g).to(cuda, dtype)                       # every row its own data
    gu = torch.randn(8, 2 * K, generator=g).to(cuda, dtype)
    res = torch.randn(8, N, generator=g).to(cuda, dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda, dtype)
    nw = (torch.randn(K, generator=g) * 0.2 + 1).to(cuda, dtype)
    return w, x, gu, res, b, nw


def _forms(x, gu, res, b, nw):
    """name -> (activation rows, bias, keyword arguments with per-row operands as [8, ...] tensors)"""
    return {"bias": (x, b, {}), "norm": (x, None, {"norm": (nw, 1e-5)}), "residual": (x, None, {"residual": res}),
            "glu_residual": (gu, None, {"glu": True, "residual": res})}


def _check_rows(single, rows, x, gu, res, b, nw):
    """``single(xrow, bias, **kw)`` / ``rows(xrows, bias, **kw)``: every form, every B; then a NaN / Inf row beside the others."""
    for name, (act, bias, kw) in _forms(x, gu, res, b, nw).items():
        def one(a, r):
            k1 = dict(kw)
            if "residual" in k1:
                k1["residual"] = k1["residual"][r]
            return single(a[r], bias, **k1)
        want = torch.stack([one(act, r) for r in range(8)])
        assert bool(torch.isfinite(want).all())
        for B in ROWS:
            kb = dict(kw)
            if "residual" in kb:
                kb["residual"] = kb["residual"][:B].contiguous()
            got = rows(act[:B].contiguous(), bias, **kb)
            assert got.shape == want[:B].shape and torch.equal(got, want[:B]), (name, B)
        for B, bad_row, bad in ((3, 1, float("nan")), (8, 6, float("inf"))):      # a poisoned row stays in its own accumulators
            a = act[:B].clone()
            a[bad_row] = bad
            kb = dict(kw)
            if "residual" in kb:
                kb["residual"] = kb["residual"][:B].contiguous()
            got = rows(a, bias, **kb)
            keep = [r for r in range(B) if r != bad_row]
            assert torch.equal(got[keep], want[keep]), (name, B, "rows beside a non-finite one changed")
            assert not bool(torch.isfinite(got[bad_row]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", NATIVE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gemv_rows_equal_the_single_row_kernel(cuda, dtype, shape):
    from rsvld_amd import decode_rows as DR, ops
    w, x, gu, res, b, nw = _operands(cuda, *shape, dtype)
    _check_rows(lambda a, bias, **kw: ops.gemv_fused(w, a, bias, **kw), lambda a, bias, **kw: DR.gemv_rows(w, a, bias, **kw),
                x, gu, res, b, nw)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", W8_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gemv_w8_rows_equal_the_single_row_kernel(cuda, dtype, shape):
    from rsvld_amd import decode_rows as DR, w8
    w, x, gu, res, b, nw = _operands(cuda, *shape, dtype)
    q, scale = w8.pack_rows_e4m3(w)
    _check_rows(lambda a, bias, **kw: w8.gemv_w8(q, scale, a, bias, **kw), lambda a, bias, **kw: DR.gemv_w8_rows(q, scale, a, bias, **kw),
                x, gu, res, b, nw)


@pytest.mark.parametrize("positions", [(0, 128, 300), (383, 5, 200)], ids=["0_128_300", "last_slot"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
def test_decode_attention_rows_equal_single_calls_on_copies(cuda, dtype, positions):
    """``_seeded_llama``'s geometry: 8 query heads on 2 kv heads, head dim 128, a cache of 384 positions (three key chunks)."""
    from rsvld_amd import decode_rows as DR, ops
    n_q, n_kv, hd, max_len, B = 8, 2, 128, 384, len(positions)
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, (n_q + 2 * n_kv) * hd, generator=g).to(cuda, dtype)
    ang = torch.rand(B, hd, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(cuda, dtype), torch.sin(ang).to(cuda, dtype)
    kc = torch.randn(B, n_kv, max_len, hd, generator=g).to(cuda, dtype)
    vc = torch.randn(B, n_kv, max_len, hd, generator=g).to(cuda, dtype)
    pos = torch.tensor(positions, device=cuda)
    scale = hd ** -0.5
    want, wk, wv = [], [], []
    for b in range(B):
        k1, v1 = kc[b].clone(), vc[b].clone()
        want.append(ops.llama_decode_attention(qkv[b], cos[b], sin[b], pos[b:b + 1].clone(), k1, v1, n_q, n_kv, scale))
        wk.append(k1)
        wv.append(v1)
    kb, vb = kc.clone(), vc.clone()
    got = DR.llama_decode_attention_rows(qkv, cos, sin, pos, kb, vb, n_q, n_kv, scale)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, torch.stack(want))
    assert torch.equal(kb, torch.stack(wk)) and torch.equal(vb, torch.stack(wv))
    for cache, orig in ((kb, kc), (vb, vc)):                   # a sequence writes its own slot only
        changed = (cache != orig).any(dim=-1)                  # [B, n_kv, max_len]
        for b in range(B):
            assert changed[b].any(dim=0).nonzero().flatten().tolist() == [positions[b]]


# ----------------------------------------------------------------------------- the batched token loop
PROMPTS, NEW, MAX_LEN = (5, 131, 300), 24, 512


@pytest.fixture(scope="module")
def llama(cuda):
    model, cfg = _seeded_llama(cuda, layers=2)
    embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(cuda))
            .detach() for n in PROMPTS]
    return model, embs


@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_generate_batch_equals_three_generate_runs(cuda, llama, weights):
    """Greedy, sampled (temperature 0.7, seeds 1 / 2 / 3; the single runs under fork_rng + manual_seed) and an early end token; through
    the captured graph and eagerly; the caller's generators are where they were."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    seeds = [1, 2, 3]
    dec1 = LN.FastDecoder(model, MAX_LEN, weights=weights)
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
    del dec1

    decb = LN.FastDecoder(model, MAX_LEN, weights=weights, batch=3)
    assert decb.k[0].shape == (3, 2, MAX_LEN, 128)
    for use_graph in (True, False):
        got = decb.generate_batch(embs, NEW, do_sample=False, use_graph=use_graph)
        assert [t.tolist() for t in got] == [t.tolist() for t in greedy], ("greedy", use_graph)
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(cuda)
        got = decb.generate_batch(embs, NEW, do_sample=True, temperature=0.7, seeds=seeds, use_graph=use_graph)
        assert [t.tolist() for t in got] == [t.tolist() for t in sampled], ("sampled", use_graph)
        assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(cuda), dev_state)
        got = decb.generate_batch(embs, NEW, do_sample=False, eos_token_id=eos, use_graph=use_graph)
        assert [t.tolist() for t in got] == [t.tolist() for t in ended], ("eos", use_graph)
    assert set(decb._rows) == {3} and decb._graph is None       # one capture per number of rows; the single-row graph was never needed
    two = decb.generate_batch(embs[1:], NEW, do_sample=False)   # fewer prompts than rows, in other cache rows than before
    assert [t.tolist() for t in two] == [t.tolist() for t in greedy[1:]]
    with pytest.raises(ValueError):
        decb.generate_batch(embs + embs[:1], NEW)
    with pytest.raises(ValueError):
        LN.FastDecoder(model, MAX_LEN, batch=9)


def test_generate_batch_with_growing_and_shrinking_row_counts(cuda, llama):
    """2, then 3, then 2 prompts on ONE decoder, the allocator's cache emptied in between (as ``ImageBatchProcessor`` does after a group):
    the step captured for two rows is replayed after the three-row one was captured, and must still read and write live memory -- the
    attention workspace is allocated once for ``batch`` rows and every captured step holds that one address."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    dec1 = LN.FastDecoder(model, MAX_LEN)
    greedy = [dec1.generate(e, NEW, do_sample=False).tolist() for e in embs]
    del dec1
    decb = LN.FastDecoder(model, MAX_LEN, batch=3)
    first_ws = None
    for rows in ((0, 1), (0, 1, 2), (1, 2), (2, 0)):
        got = decb.generate_batch([embs[r] for r in rows], NEW, do_sample=False)
        assert [t.tolist() for t in got] == [greedy[r] for r in rows], rows
        ws = decb._ws_rows
        torch.cuda.empty_cache()
        assert first_ws is None or ws is first_ws, "the workspace was replaced under a captured step"
        first_ws = ws
    assert set(decb._rows) == {2, 3}


def test_generate_on_a_batch_decoder_touches_its_own_cache_row_only(cuda, llama):
    """``generate`` is the decode step on ONE row of a ``batch=3`` decoder (cache row ``_row`` = 0): rows 1 and 2 of every layer's caches
    keep their bits, through the captured graph and eagerly, and row 0 is what was written."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    decb = LN.FastDecoder(model, MAX_LEN, batch=3)
    g = torch.Generator().manual_seed(5)
    for c in decb.k + decb.v:
        c.copy_(torch.randn(c.shape, generator=g).to(cuda, c.dtype))
    before = [c.clone() for c in decb.k + decb.v]
    assert decb._row == 0
    for use_graph in (True, False):
        toks = decb.generate(embs[1], NEW, do_sample=False, use_graph=use_graph)
        assert len(toks) == NEW
    for c, c0 in zip(decb.k + decb.v, before):
        assert torch.equal(c[1:], c0[1:]), "generate wrote outside cache row 0"
        assert not torch.equal(c[0, :, :PROMPTS[1] + NEW - 1], c0[0, :, :PROMPTS[1] + NEW - 1])


def test_generate_and_generate_batch_share_one_workspace(cuda, llama):
    """A graph-captured ``generate``, a ``generate_batch`` of three, then ``generate`` again on ONE decoder: the single-row graph replays
    after the three-row step used the same attention workspace, and gives the tokens of a fresh ``batch=1`` decoder."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    dec1 = LN.FastDecoder(model, MAX_LEN)
    greedy = [dec1.generate(e, NEW, do_sample=False).tolist() for e in embs]
    del dec1
    decb = LN.FastDecoder(model, MAX_LEN, batch=3)
    assert decb.generate(embs[2], NEW, do_sample=False).tolist() == greedy[2]
    ws = decb._ws_rows
    assert decb._graph is not None and ws is not None
    assert [t.tolist() for t in decb.generate_batch(embs, NEW, do_sample=False)] == greedy
    torch.cuda.empty_cache()
    assert decb.generate(embs[1], NEW, do_sample=False).tolist() == greedy[1]
    assert decb._ws_rows is ws and set(decb._rows) == {3}, "the workspace was replaced under a captured step"


def test_a_finished_row_draws_nothing_from_a_shared_generator(cuda, llama):
    """``seeds=None``: every row samples from the caller's default generator.  Row 0 ends with its first token, so the batch is one draw
    for row 0 followed by row 1's draws -- what two single calls in a row draw (one new token for prompt 0, then prompt 1 in full).  A
    finished row that went on drawing would shift row 1's draws."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    dec1 = LN.FastDecoder(model, MAX_LEN)
    with torch.random.fork_rng(devices=[cuda]):
        torch.manual_seed(9)
        head = dec1.generate(embs[0], 1, do_sample=True, temperature=0.7)
        tail = dec1.generate(embs[1], NEW, do_sample=True, temperature=0.7)
    eos = int(head[0])
    assert len(tail) == NEW and eos not in tail.tolist(), "row 1 must outlive row 0 for the case to show anything"
    del dec1
    decb = LN.FastDecoder(model, MAX_LEN, batch=2)
    with torch.random.fork_rng(devices=[cuda]):
        torch.manual_seed(9)
        got = decb.generate_batch(embs[:2], NEW, do_sample=True, temperature=0.7, eos_token_id=eos)
    assert got[0].tolist() == head.tolist() and got[1].tolist() == tail.tolist()
