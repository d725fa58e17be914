"""A-B of the caption pass's PREFILL with its attention as the stock-torch sequence (``FastDecoder(prefill="torch")``, the default) against
the causal grouped-query flash kernel (``prefill="flash"``, ``--caption_prefill flash``; csrc/prefill_attention.hip), in ONE process on
one device: the full-size seeded 8 B decoder of tools/synthetic_models.py behind a prompt of the bench's length (3 047 positions:
profiles/r06_bench_c4.json), cache length 3 328.

  * prefill: ``FastDecoder.profile["prefill_s"]`` (device-synchronised wall time of ``forward`` on the prompt plus the first pick), the
    two routes alternating -- T F T F T F, then F T F T F T: six pairs, three in each order -- per pair and as medians;
  * peak memory: ``torch.cuda.max_memory_allocated`` across each prefill, above what was allocated before it;
  * the attention kernel alone: us per launch (= per layer) by device events around a batch of launches, and the TFLOP/s that implies on
    2 * 2 * n_q * 128 * T^2 / 2 FLOP; the torch sequence of one layer (scores, softmax, PV over the whole cache) the same way;
  * max |difference| of the two routes' prefill logits (information: the routes round differently, tests/test_gpu_caption_prefill.py).

There is no threshold here: the numbers are written down, not met.

    python tools/bench_caption_prefill.py --out profiles/caption_prefill_ab.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _median(v):
    return sorted(v)[len(v) // 2]


def _time_us(fn, iters, repeats):
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return _median(out), min(out), max(out)


def attention_alone(dev, log, T, n_q, n_kv, max_len, iters=10, repeats=5):
    """One layer's attention at the prompt's shape: the kernel, and the torch sequence of ``FastDecoder.forward``."""
    from rsvld_amd import prefill_attention as PA
    hd, g = 128, n_q // n_kv
    gen = torch.Generator(device=dev).manual_seed(3)
    qk = torch.randn(T, n_q + n_kv, hd, device=dev, dtype=torch.float16, generator=gen)
    kc = torch.randn(n_kv, max_len, hd, device=dev, dtype=torch.float16, generator=gen)
    vc = torch.randn(n_kv, max_len, hd, device=dev, dtype=torch.float16, generator=gen)
    scale = hd ** -0.5
    flops = 2.0 * 2.0 * n_q * hd * T * T / 2.0
    pl = PA.plan(T, n_q, n_kv)
    med, lo, hi = _time_us(lambda: PA.llama_prefill_attention(qk[:, :n_q], kc, vc, n_q, n_kv, scale, pos0=0), iters, repeats)
    log(f"flash kernel: grid {pl.grid_x} x {pl.grid_y} = {pl.grid_x * pl.grid_y} workgroups; {med:.1f} us per launch (= per layer; "
        f"min {lo:.1f}, max {hi:.1f} over {repeats} batches of {iters}) = {flops / med * 1e-6:.1f} TFLOP/s on {flops * 1e-12:.3f} TFLOP "
        f"(2 * 2 * n_q * 128 * T^2 / 2); 32 layers: {32 * med * 1e-3:.2f} ms")
    pos = torch.arange(T, device=dev)
    cols = torch.arange(max_len, device=dev)

    def torch_route():
        bias = torch.zeros((T, max_len), device=dev, dtype=torch.float32)
        bias.masked_fill_(cols[None, :] > pos[:, None], float("-inf"))
        q = qk[:, :n_q].reshape(T, n_kv, g, hd).permute(1, 0, 2, 3).reshape(n_kv, T * g, hd)
        sc = torch.matmul(q, kc.transpose(1, 2)).float().view(n_kv, T, g, max_len)
        pr = torch.softmax(sc * scale + bias[None, :, None, :], dim=-1).to(torch.float16).view(n_kv, T * g, max_len)
        return torch.matmul(pr, vc).view(n_kv, T, g, hd).permute(1, 0, 2, 3).reshape(T, n_q * hd)
    med_t, lo_t, hi_t = _time_us(torch_route, max(1, iters // 5), repeats)
    log(f"torch sequence of one layer (mask, scores over {max_len} slots, fp32 softmax, PV; the mask is built once per prefill, here per "
        f"call): {med_t:.1f} us (min {lo_t:.1f}, max {hi_t:.1f}); 32 layers: {32 * med_t * 1e-3:.2f} ms")
    return med, med_t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=256, help="sizes the cache only (prompt + new tokens, rounded up to 256)")
    ap.add_argument("--pairs", type=int, default=3, help="pairs per order (>= 3 in all)")
    ap.add_argument("--kernel_only", action="store_true", help="only the attention of one layer (no model is built)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_caption_prefill: no GPU visible (a measurement needs one; there is no CPU stand-in)")
    dev = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
    log(f"# caption prefill, attention as the torch sequence vs the causal flash kernel: {torch.cuda.get_device_name(0)}, 8 B decoder "
        f"(seeded, fp16), prompt {a.prompt}, cache length {max_len}")
    log("\n## the attention of one layer alone (32 query heads on 8 kv heads, head_dim 128; device events)")
    attention_alone(dev, log, a.prompt, 32, 8, max_len)
    save()
    if a.kernel_only:
        return
    from rsvld_amd import llava_next as LN
    from tools import synthetic_models as SM
    model = SM.llava_full(dev)[0]
    with torch.no_grad():
        emb = model.model.embed_tokens(torch.randint(1000, 100000, (1, a.prompt), generator=torch.Generator().manual_seed(7)).to(dev))
        decs = {m: LN.FastDecoder(model, max_len, prefill=m) for m in ("torch", "flash")}

        def prefill(mode):
            """-> (prefill ms, peak MiB above the allocation in front of the prefill, first token)"""
            dec = decs[mode]
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            dec.profile = {}
            tok = dec.generate(emb, 1, do_sample=False, use_graph=False)
            p, dec.profile = dec.profile, None
            return p["prefill_s"] * 1e3, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, tok

        for m in decs:                                              # warm-up: allocator, library algorithm choices, code objects
            prefill(m)
            prefill(m)
        lt = decs["torch"].forward(emb.to(torch.float16), torch.arange(a.prompt, device=dev), pos0=0).float()
        lf = decs["flash"].forward(emb.to(torch.float16), torch.arange(a.prompt, device=dev), pos0=0).float()
        log(f"\n## prefill logits of the two routes at this prompt: max |flash - torch| = {float((lf - lt).abs().max()):.3e} "
            f"(max |torch| = {float(lt.abs().max()):.3e}); argmax equal: {bool(lf.argmax() == lt.argmax())}")
        log("\n## prefill_s (FastDecoder.profile) and peak memory across the prefill, alternating pairs")
        ms, mib = {"torch": [], "flash": []}, {"torch": [], "flash": []}
        for n, order in enumerate((("torch", "flash"),) * a.pairs + (("flash", "torch"),) * a.pairs):
            got = {}
            for m in order:
                got[m] = prefill(m)
                ms[m].append(got[m][0])
                mib[m].append(got[m][1])
            log(f"pair {n + 1} ({order[0]} first): torch {got['torch'][0]:8.2f} ms {got['torch'][1]:8.0f} MiB | flash {got['flash'][0]:8.2f} ms "
                f"{got['flash'][1]:8.0f} MiB | flash / torch = {got['flash'][0] / got['torch'][0]:.3f}")
        mt, mf = _median(ms["torch"]), _median(ms["flash"])
        log(f"\nmedian prefill: torch {mt:.2f} ms, flash {mf:.2f} ms, flash / torch = {mf / mt:.3f}; flash faster in "
            f"{sum(f < t for f, t in zip(ms['flash'], ms['torch']))} of {len(ms['torch'])} pairs")
        log(f"median peak memory across the prefill: torch {_median(mib['torch']):.0f} MiB, flash {_median(mib['flash']):.0f} MiB")
    save()


if __name__ == "__main__":
    main()
