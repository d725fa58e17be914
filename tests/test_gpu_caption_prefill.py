"""``FastDecoder(prefill="flash")``: the caption pass's prefill through rsvld_amd.prefill_attention on the seeded Llama of
tests/test_gpu_w8.py (2 layers, 8 heads on 2 kv heads, head_dim 128) and prompts of 5, 131 and 300 embeddings.

* Distance from an fp32 CPU run of the same forward (the same weights widened, the torch route in fp32): the flash route keeps fp32
  scores where the torch route rounds them to 16 bits, so its prefill logits must not be further from that reference than twice the
  torch route's (the factor covers the scatter of a maximum over 2 000 logits).  Tokens of the two routes are NOT compared: the seeded
  model's logits are nearly flat.
* Within the flash route, ``torch.equal``: prefill logits, the written cache rows and the tokens do not depend on ``max_len``; a batched
  caption equals the single captions of a decoder BUILT AT ANOTHER ``max_len`` (the case the torch prefill's Condition excludes), greedy
  and sampled; the e4m3 mode runs with it; what an earlier, longer prompt left in the cache does not reach a shorter one."""
import copy

import pytest
import torch

from test_gpu_w8 import _seeded_llama

pytestmark = pytest.mark.gpu

PROMPTS, NEW = (5, 131, 300), 24


@pytest.fixture(scope="module")
def llama(cuda):
    model, cfg = _seeded_llama(cuda, layers=2)
    embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(cuda))
            .detach() for n in PROMPTS]
    return model, embs


def _prefill(dec, emb):
    """-> the prefill's logits [1, vocab]; the cache rows 0 .. T - 1 of cache row 0 are written."""
    with torch.no_grad():
        return dec.forward(emb.to(dec.dt), torch.arange(emb.shape[1], device=dec.dev), pos0=0)


def _cache_rows(dec, T):
    return [c[0][:, :T].clone() for c in dec.k + dec.v]


def test_flash_prefill_is_no_further_from_an_fp32_run_than_the_torch_prefill(cuda, llama):
    """e_flash <= 2 e_torch (max |logit difference| from the fp32 CPU run over the three prompts).  Measured on an MI355X (fp16):
    e_flash = 3.474e-02, e_torch = 3.000e-02 -- the two routes are equally far; what separates either from the fp32 run is the 16-bit
    rounding of the projections, not the scores (profiles/caption_prefill_ab.txt)."""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    ref_model = copy.deepcopy(model).to(device="cpu", dtype=torch.float32)
    ref = LN.FastDecoder(ref_model, 512)                                      # the torch route, eagerly, in fp32 on the host
    want = [_prefill(ref, e.cpu().float()) for e in embs]
    err = {}
    for mode in ("torch", "flash"):
        dec = LN.FastDecoder(model, 512, prefill=mode)
        err[mode] = max(float((_prefill(dec, e).float().cpu() - w).abs().max()) for e, w in zip(embs, want))
    print(f"caption prefill, max|logits - fp32 CPU run| over prompts {PROMPTS}: e_flash = {err['flash']:.3e}, e_torch = {err['torch']:.3e}")
    assert err["torch"] > 0
    assert err["flash"] <= 2 * err["torch"], err


def test_flash_prefill_and_its_tokens_do_not_depend_on_max_len(cuda, llama):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    a, b = LN.FastDecoder(model, 512, prefill="flash"), LN.FastDecoder(model, 768, prefill="flash")
    for e in embs:
        T = e.shape[1]
        la, lb = _prefill(a, e), _prefill(b, e)
        assert torch.equal(la, lb), T
        for ca, cb in zip(_cache_rows(a, T), _cache_rows(b, T)):
            assert torch.equal(ca, cb), T
        assert a.generate(e, NEW, do_sample=False).tolist() == b.generate(e, NEW, do_sample=False).tolist(), T


@pytest.mark.parametrize("weights", ["native", "e4m3"])
def test_batched_flash_caption_equals_single_captions_at_another_max_len(cuda, llama, weights):
    """``generate_batch`` of a batch-3 decoder at max_len 512 against three ``generate`` runs of a batch-1 decoder at max_len 768: greedy,
    and sampled under seeds 1 / 2 / 3.  (e4m3: the mode runs with the flash prefill and equals its own single-row runs.)"""
    from rsvld_amd import llava_next as LN
    model, embs = llama
    seeds = [1, 2, 3]
    dec1 = LN.FastDecoder(model, 768, weights=weights, prefill="flash")
    greedy = [dec1.generate(e, NEW, do_sample=False) for e in embs]
    sampled = []
    for e, s in zip(embs, seeds):
        with torch.random.fork_rng(devices=[cuda]):
            torch.manual_seed(s)
            sampled.append(dec1.generate(e, NEW, do_sample=True, temperature=0.7))
    del dec1
    decb = LN.FastDecoder(model, 512, weights=weights, batch=3, prefill="flash")
    got = decb.generate_batch(embs, NEW, do_sample=False)
    assert [t.tolist() for t in got] == [t.tolist() for t in greedy]
    got = decb.generate_batch(embs, NEW, do_sample=True, temperature=0.7, seeds=seeds)
    assert [t.tolist() for t in got] == [t.tolist() for t in sampled]
    assert all(len(t) == NEW for t in greedy + sampled)


def test_a_shorter_prompt_does_not_see_what_a_longer_one_left_in_the_cache(cuda, llama):
    from rsvld_amd import llava_next as LN
    model, embs = llama
    used = LN.FastDecoder(model, 512, prefill="flash")
    _prefill(used, embs[2])                                                   # 300 positions of every cache row filled
    fresh = LN.FastDecoder(model, 512, prefill="flash")
    for e in embs[:2]:
        assert torch.equal(_prefill(used, e), _prefill(fresh, e)), e.shape[1]
    # ... nor NaN in the slots above the prompt
    for c in fresh.k + fresh.v:
        c[:, :, 131:] = float("nan")
    assert torch.equal(_prefill(fresh, embs[1]), _prefill(used, embs[1]))


def test_flash_refuses_what_the_kernel_does_not_cover(cuda, llama):
    from rsvld_amd import llava_next as LN
    model, _ = llama
    with pytest.raises(ValueError, match="flash"):
        LN.FastDecoder(copy.deepcopy(model).float(), 512, prefill="flash")    # fp32 weights
    dec = LN.FastDecoder(model, 512, prefill="flash")
    with pytest.raises(ValueError, match="pos0"):
        dec.forward(torch.zeros(1, 4, 1024, device=cuda, dtype=dec.dt), torch.arange(4, device=cuda))
