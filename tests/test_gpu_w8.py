"""rsvld_amd/w8.py on the GPU: the e4m3 row quantiser against its host model bit for bit, the e4m3 weight-streaming GEMV on exactly
computable operands bit for bit against fp64 and on random operands inside the 16-bit GEMV's own bound, and the token loop of
``FastDecoder(weights="e4m3")`` against the native loop on e4m3-exact weights.

The generators (``edge_rows``, ``build_exact``) assert their own premises; tests/test_w8_cases.py walks them on the CPU."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}


# ----------------------------------------------------------------------------- rows for the quantiser
def _step(v, dtype, n):
    """The value ``n`` representable steps away from ``v`` in ``dtype`` (positive finite ``v``)."""
    t = torch.tensor([v], dtype=dtype)
    assert float(t) == v, (v, dtype)
    return float((t.view(torch.int16) + n).view(dtype))


def edge_rows(dtype, K=48, nonfinite=False):
    """-> ``(w [N, K] in dtype, names)``: rows whose amax is 448 * 2^j (m = 0.875 exactly: the last amax that keeps the smaller exponent),
    its two neighbours in ``dtype`` (m just below / just above 0.875), powers of two (m = 0.5), an all-zero row, a row of 16-bit
    subnormals, rows of N(0, 0.02) weights; ``nonfinite``: plus a row holding a NaN and an Inf among ordinary weights."""
    g = torch.Generator().manual_seed(48)
    rows, names = [], []

    def add(name, amax, fill=0.3):
        r = (torch.rand(K, generator=g) * 2 - 1) * fill * amax
        r[int(torch.randint(0, K, (1,), generator=g))] = amax * (1 if len(rows) % 2 else -1)
        rows.append(r.to(dtype))
        names.append(name)

    for j in ((-20, -8, 0, 7) if dtype == torch.float16 else (-130, -20, 0, 100, 119)):
        a = math.ldexp(448.0, j)
        add(f"448*2^{j}", a)
        add(f"448*2^{j}-", _step(a, dtype, -1))
        add(f"448*2^{j}+", _step(a, dtype, +1))
        add(f"2^{j}", math.ldexp(1.0, j))
    rows.append(torch.zeros(K, dtype=dtype))
    names.append("zero")
    nsub = 1023 if dtype == torch.float16 else 127            # the largest subnormal's bit pattern
    sub = torch.randint(-nsub, nsub + 1, (K,), generator=g).to(torch.int16)
    sub = torch.where(sub < 0, (-sub) | torch.tensor(-32768, dtype=torch.int16), sub).view(dtype)
    rows.append(sub)
    names.append("subnormals")
    rows.append(torch.full((K,), float(torch.tensor([1], dtype=torch.int16).view(dtype)), dtype=dtype))
    names.append("smallest_subnormal")
    for i in range(4):
        rows.append((torch.randn(K, generator=g) * 0.02).to(dtype))
        names.append(f"normal{i}")
    if nonfinite:
        r = (torch.randn(K, generator=g) * 0.02).to(dtype)
        r[3], r[K // 2 + 1], r[K - 1] = float("nan"), float("inf"), float("-inf")
        rows.append(r)
        names.append("nan_inf")
    w = torch.stack(rows)
    sub_row = w[names.index("subnormals")].float().abs()
    assert float(sub_row.max()) < (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126) and float(sub_row.max()) > 0
    assert not nonfinite or int((~torch.isfinite(w.float())).sum()) == 3
    return w, names


def brute_force_exponent(amax):
    """The smallest integer e with amax * 2^-e <= 448 (exact in Python's doubles), 0 for amax = 0, clamped to [-126, 127]."""
    if amax == 0:
        return 0
    e = -300
    while math.ldexp(amax, -e) > 448.0:
        e += 1
    assert math.ldexp(amax, -e) <= 448.0 < math.ldexp(amax, -(e - 1))
    return min(max(e, -126), 127)


# ----------------------------------------------------------------------------- exactly computable GEMV operands
# (N, K) and the branch of rsvld_gemv_w8_fused each takes (csrc/gemv.hip: ksplit = K % 64 == 0 && K >= 2048 && ceil(N / 16) < 1024;
# the main loop takes whole 2 048-element double steps of a wave's K range, the tail loop 1 024-element steps with pieces past the end
# skipped per lane):
EXACT_SHAPES = [
    (17, 16),        # row route (K < 2 048), 2 workgroups: the tail loop once with ONE lane active; wave 0 of workgroup 1 owns row 16 and
                     #   three rows past N (re-read, never stored), its other waves leave at once
    (1003, 528),     # row route (528 % 64 = 16): the tail loop once, lanes 0 .. 32 (one 16-element piece past 512); 1003 = 62 x 16 + 11: ragged N
    (6, 4096),       # K-split route, 2 workgroups of 4 rows (two past N): a wave's quarter is 1 024 = no double step, ONE whole tail step
    (6, 14336),      # K-split route, a quarter is 3 584 = 3.5 steps (down_proj): one double step, one whole tail step, one with lanes 0 .. 31
    (16400, 2048),   # row route although K is split-eligible (ceil(16 400 / 16) = 1 025 workgroups >= 1 024): one double step, no tail
]


def build_exact(dtype, N, K):
    """Operands whose product, bias and residual are exact at every step of the kernel AND of an fp64 reference:
    * weights u * 2^t[n] with integers |u| <= 7 and row exponents t[n] in -2 .. 3: e4m3-exact (asserted: the host quantiser gives them
      back), so the rows' scales differ;
    * x: 16 non-zero small integers (|x| <= 2) -- first and last element of K, both ends of every K quarter, the rest at random --
      zeros elsewhere: |sum| <= 16 * 2 * 7 = 224 in units of 2^t;
    * bias and residual: integers |.| <= 15 in the same units, so every intermediate has at most 8 significant bits (bf16's) and every
      fp32 partial sum over the e4m3 integers stays far below 2^24."""
    from rsvld_amd import w8
    g = torch.Generator().manual_seed(N * 31 + K)
    t = torch.randint(-2, 4, (N,), generator=g)
    t[:6] = torch.tensor([-2, -1, 0, 1, 2, 3])[:min(N, 6)]
    unit = torch.ldexp(torch.ones(N, dtype=torch.float64), t)
    u = torch.randint(-7, 8, (N, K), generator=g)
    w = (u.double() * unit[:, None]).to(dtype)
    x = torch.zeros(K, dtype=torch.float64)
    q4 = K // 4
    forced = sorted({0, K - 1} | {min(max(p, 0), K - 1) for i in range(1, 4) for p in (i * q4 - 1, i * q4)})
    rest = torch.randperm(K, generator=g)[:16 - len(forced)].tolist()
    for p in forced + rest:
        x[p] = float(torch.randint(1, 3, (1,), generator=g)) * (1 if int(torch.randint(0, 2, (1,), generator=g)) else -1)
    bias = torch.randint(-15, 16, (N,), generator=g).double() * unit
    res = torch.randint(-15, 16, (N,), generator=g).double() * unit
    # premises
    assert torch.equal(w.double(), u.double() * unit[:, None])
    q, scale = w8.pack_rows_e4m3_host(w)
    dq = w8.dequant(q, scale)
    assert torch.equal(dq.double(), w.double()), "weights are not e4m3-exact"
    assert len(set(scale.tolist())) > 1 or N == 1, "row exponents do not differ"
    qi = q.view(torch.float8_e4m3fn).float()
    assert torch.equal(qi, qi.round()) and int(x.count_nonzero()) <= 16
    assert float((qi.abs().double() @ x.abs()).max()) < 2 ** 24
    prod = w.double() @ x
    stages = {"plain": prod, "bias": prod + bias, "bias_res": (prod + bias).to(dtype).double() + res}
    for name, v in stages.items():
        assert torch.equal(v.to(dtype).double(), v), f"{name}: not representable in {dtype}"
    return dict(w=w, q=q, scale=scale, x=x.to(dtype), bias=bias.to(dtype), res=res.to(dtype),
                want={k: v.to(dtype) for k, v in stages.items()})


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
def test_pack_rows_equals_the_host_model(cuda, dtype):
    from rsvld_amd import w8
    for K in (16, 48, 2064):         # one piece; three pieces (lanes 0 .. 2); more than one wave step with a ragged last one
        w, names = edge_rows(dtype, K, nonfinite=True)
        q, scale = w8.pack_rows_e4m3(w.to(cuda))
        qh, sh = w8.pack_rows_e4m3_host(w)
        bad = [n for i, n in enumerate(names) if not torch.equal(q[i].cpu(), qh[i]) or float(scale[i]) != float(sh[i])]
        assert not bad, (K, bad)
        assert torch.equal(q.cpu(), qh) and torch.equal(scale.cpu(), sh)
        assert int((qh[names.index("nan_inf")] == w8.E4M3_NAN).sum()) == 3


# ----------------------------------------------------------------------------- GEMV
@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gemv_w8_exact_operands(cuda, dtype, shape):
    """Bit for bit against fp64, through the device quantiser (which must return the host model's bytes for these rows)."""
    from rsvld_amd import w8
    c = build_exact(dtype, *shape)
    q, scale = w8.pack_rows_e4m3(c["w"].to(cuda))
    assert torch.equal(q.cpu(), c["q"]) and torch.equal(scale.cpu(), c["scale"])
    x, b, r = c["x"].to(cuda), c["bias"].to(cuda), c["res"].to(cuda)
    assert torch.equal(w8.gemv_w8(q, scale, x).cpu(), c["want"]["plain"])
    assert torch.equal(w8.gemv_w8(q, scale, x, b).cpu(), c["want"]["bias"])
    assert torch.equal(w8.gemv_w8(q, scale, x, b, residual=r).cpu(), c["want"]["bias_res"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", [(4096, 4096), (6144, 4096), (28672, 4096), (4096, 14336), (1003, 528), (17, 16)])
def test_gemv_w8_weight_streaming(cuda, dtype, shape):
    """The decode-step shapes of Llama-3-8B, ragged N and K: against the fp64 product over ``dequant(q, scale)`` -- after dequantisation
    the arithmetic is the 16-bit kernel's own, so tests/test_gpu_kernels.py's bound applies unchanged."""
    from rsvld_amd import w8
    N, K = shape
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dtype)
    x = torch.randn(K, generator=g).to(cuda, dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda, dtype)
    q, scale = w8.pack_rows_e4m3(w)
    dq = w8.dequant(q, scale).double()
    aw, sc = w.double().abs(), scale.double()[:, None]
    bound = torch.where(aw >= sc * 2.0 ** -6, aw * 2.0 ** -4, sc * 2.0 ** -10)     # the quantiser's own bound (normal / subnormal e4m3)
    assert bool(((dq - w.double()).abs() <= bound).all())
    want = (dq @ x.double()).float().cpu()
    _close(w8.gemv_w8(q, scale, x), want, dtype)
    _close(w8.gemv_w8(q, scale, x, b), want + b.float().cpu(), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", [(6144, 4096), (4096, 14336), (1003, 528)])
def test_gemv_w8_fused_decode_step_neighbours(cuda, dtype, shape):
    """The RMSNorm prologue, the SwiGLU prologue and the residual epilogue, each against the unfused torch sequence on the dequantised
    weights and the torch-staged x' (as test_gemv_fused_decode_step_neighbours does for the 16-bit kernel)."""
    from rsvld_amd import w8
    N, K = shape
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda, dtype)
    x = (torch.randn(K, generator=g) * 2).to(cuda, dtype)
    nw = (torch.randn(K, generator=g) * 0.2 + 1).to(cuda, dtype)
    res = torch.randn(N, generator=g).to(cuda, dtype)
    gu = torch.randn(2 * K, generator=g).to(cuda, dtype)
    q, scale = w8.pack_rows_e4m3(w)
    dq = w8.dequant(q, scale).double()
    lin = lambda v: (dq @ v.double()).to(dtype)        # the product's fp32 accumulation, rounded once
    want_n = lin(F.rms_norm(x, (K,), nw, 1e-5))
    want_r = res + lin(x)
    want_g = res + lin(F.silu(gu[:K]) * gu[K:])
    _close(w8.gemv_w8(q, scale, x, None, norm=(nw, 1e-5)), want_n.float().cpu(), dtype)
    _close(w8.gemv_w8(q, scale, x, None, residual=res), want_r.float().cpu(), dtype)
    _close(w8.gemv_w8(q, scale, gu, None, glu=True, residual=res), want_g.float().cpu(), dtype)


# ----------------------------------------------------------------------------- decoder
def _seeded_llama(cuda, intermediate=2048, layers=3):
    """The seeded Llama of test_fast_decoder_fused_decode_step_equals_the_torch_sequence (tests/test_gpu_infer.py)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=2000, hidden_size=1024, intermediate_size=intermediate, num_hidden_layers=layers, num_attention_heads=8,
                      num_key_value_heads=2, max_position_embeddings=1024, rms_norm_eps=1e-5, rope_theta=500000.0, attention_bias=False)
    torch.manual_seed(11)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p_ in model.parameters():                    # a spread of magnitudes instead of the uniform init
            p_.mul_(2.0)
    return model.to(device=cuda, dtype=torch.float16), cfg


def _dequantised_copy(model):
    """A copy whose eight kinds of weight tensors (q, k, v, o, gate, up, down of every layer; lm_head) hold dequant(pack(w)) in fp16."""
    from rsvld_amd import w8
    twin = copy.deepcopy(model)
    with torch.no_grad():
        mats = [twin.lm_head]
        for layer in twin.model.layers:
            at, mlp = layer.self_attn, layer.mlp
            mats += [at.q_proj, at.k_proj, at.v_proj, at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj]
        for lin in mats:
            q, s = w8.pack_rows_e4m3(lin.weight.data.contiguous())
            dq = w8.dequant(q, s)
            assert torch.equal(dq.half().float(), dq)     # e4m3 x 2^e is an fp16 value here
            lin.weight.data = dq.half()
    return twin


def _teacher_forced(dec, emb, toks):
    """Prefill, then one eager decode step per token of ``toks``: -> logits ``[1 + len(toks), vocab]`` (fp32, on the host)."""
    T0 = emb.shape[1]
    embed = dec.model.model.embed_tokens
    with torch.no_grad():
        out = [dec.forward(emb.to(dec.dt), torch.arange(T0, device=dec.dev)).float().cpu()]
        for n, tok in enumerate(toks):
            out.append(dec.forward(embed(tok.view(1))[None], torch.tensor([T0 + n], device=dec.dev)).float().cpu())
    return torch.cat(out)


def test_fast_decoder_e4m3_token_loop(cuda):
    """``weights="e4m3"`` against ``weights="native"`` on a copy of the model whose weights were replaced by ``dequant(...)``: there both
    modes multiply the SAME numbers (asserted: the copy's packs dequantise to the original's, bit for bit) and differ in summation order only.
    Both decoders run on that copy, so their prefills -- which keep the 16-bit weights in either mode -- fill equal caches.  Teacher-forced
    over the 24 steps behind a 300-token prompt (across the 256-key chunk boundary); logits, not tokens, are compared (a near-tie may
    flip on summation order), within the bound of the test this model comes from.  The graph replay equals the eager steps bit for bit."""
    from rsvld_amd import llava_next as LN, w8
    model, cfg = _seeded_llama(cuda)
    twin = _dequantised_copy(model)
    ids = torch.randint(0, cfg.vocab_size, (1, 300), generator=torch.Generator().manual_seed(3)).to(cuda)
    emb = twin.model.embed_tokens(ids)
    dec_orig = LN.FastDecoder(model, 400, weights="e4m3")
    dec_g = LN.FastDecoder(twin, 400, weights="e4m3")
    for a, b in zip(dec_orig._packs[:-1] + [(dec_orig._packs[-1],)], dec_g._packs[:-1] + [(dec_g._packs[-1],)]):
        for (qa, sa), (qb, sb) in zip(a, b):
            assert torch.equal(w8.dequant(qa, sa), w8.dequant(qb, sb))      # quantising dequant(q, scale) returns its values
    del dec_orig
    with torch.no_grad():
        toks = dec_g.generate(emb, 24, do_sample=False)             # through the captured graph
    assert dec_g._graph is not None and dec_g._ws_rows is not None and len(toks) == 24
    graph_last = dec_g._logits.float().cpu()
    dec_e = LN.FastDecoder(twin, 400, weights="e4m3")
    le = _teacher_forced(dec_e, emb, toks[:-1])
    assert torch.equal(le[-1:], graph_last), "graph replay differs from the eager step"
    assert le.argmax(-1).tolist() == toks.cpu().tolist()
    dec_n = LN.FastDecoder(twin, 400)
    assert dec_n.weights == "native" and dec_n._packs is None
    ln = _teacher_forced(dec_n, emb, toks[:-1])
    assert torch.equal(le[0], ln[0])                                 # the prefill is the 16-bit one in both modes
    for n in range(1, 24):
        d, rng = float((le[n] - ln[n]).abs().max()), float(ln[n].abs().max())
        print(f"step {n}: e4m3 vs native on dequantised weights, logits max|d| = {d:.3e} (range {rng:.2f})")
        assert d < 2e-2 * rng, (n, d, rng)
    # an in-place update of a packed weight makes the decoder stale: the pack is a copy (the native decoder streams the tensor itself)
    dec_s = LN.FastDecoder(twin, 256, weights="e4m3")              # (the last decoder built on ``twin``: its fused views are the current ones)
    assert not dec_s.stale()
    with torch.no_grad():
        twin.model.layers[1].mlp.down_proj.weight.add_(0)
    assert dec_s.stale()


def test_caption_tokens_fast_rebuilds_on_mode_switch(cuda):
    from rsvld_amd import llava_next as LN
    model, cfg = _seeded_llama(cuda, layers=1)
    model.multimodal_embeds = lambda ids, images, sizes: model.model.embed_tokens(ids)
    ids = torch.randint(0, cfg.vocab_size, (1, 20), generator=torch.Generator().manual_seed(4)).to(cuda)
    run = lambda mode: LN.caption_tokens_fast(model, ids, None, None, 4, False, 1.0, None, weights=mode)
    with torch.no_grad():
        run("native")
        d0 = model._fast_decoder
        assert d0.weights == "native" and d0._graph is not None
        run("e4m3")
        d1 = model._fast_decoder
        assert d1 is not d0 and d1.weights == "e4m3" and d1._graph is not None and d1._graph is not d0._graph
        run("e4m3")
        assert model._fast_decoder is d1
        run("native")
        assert model._fast_decoder is not d1 and model._fast_decoder.weights == "native"
    with pytest.raises(ValueError):
        LN.FastDecoder(model, 256, weights="fp8")


def test_fast_decoder_e4m3_raises_on_rows_of_no_whole_pieces(cuda):
    """intermediate_size 2 056: K % 8 == 0 (the native decode step runs) but K % 16 != 0 for down_proj: no pack, no silent fallback."""
    from rsvld_amd import llava_next as LN
    model, _ = _seeded_llama(cuda, intermediate=2056, layers=1)
    LN.FastDecoder(model, 256)
    with pytest.raises(ValueError, match="K % 16"):
        LN.FastDecoder(model, 256, weights="e4m3")
