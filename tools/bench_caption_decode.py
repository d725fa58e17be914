"""A-B of the caption pass's token loop on the checkpoint's 16-bit weights ("native") against e4m3 weights with a scale per row ("e4m3",
rsvld_amd.w8), in ONE process on one device: the full-size seeded 8 B decoder of tools/synthetic_models.py, a 256-token greedy loop behind
a prompt of the bench's length (3 047 positions: profiles/r06_bench_c4.json).

  * ms per token from ``FastDecoder.profile`` (device-synchronised wall time of the loop, sampling included), the modes alternating
    N E N E, then E N E N: four pairs, two in each order;
  * GB/s of weight bytes per GEMV shape of the decoder, both kernels, over weight copies that rotate through more memory than the
    256 MB last-level cache holds;
  * under teacher forcing (the native loop's greedy tokens), the distance of the e4m3 logits from the native ones relative to the
    native logits' range, and the top-1 agreement.  Seeded random weights give nearly flat logits: this says nothing about captions.

    python tools/bench_caption_decode.py --out profiles/caption_e4m3_ab.txt      (tools/bench_caption_decode.sh: under a time limit)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("q|k|v", 6144, 4096), ("o_proj", 4096, 4096), ("gate|up", 28672, 4096), ("down_proj", 4096, 14336), ("lm_head", 128256, 4096)]
ROTATE_BYTES = 2 << 30


def gemv_rates(dev, log, iters=20, repeats=5):
    from rsvld_amd import ops, w8
    log(f"{'shape':<10} {'N':>7} {'K':>6} | {'native us':>10} {'GB/s':>7} | {'e4m3 us':>9} {'GB/s':>7} | time ratio")
    g = torch.Generator(device=dev).manual_seed(1)
    for name, N, K in SHAPES:
        ncopy = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        ws = [torch.empty(N, K, device=dev, dtype=torch.float16).normal_(0, 0.02, generator=g) for _ in range(ncopy)]
        packs = [w8.pack_rows_e4m3(w) for w in ws]
        glu = name == "down_proj"
        x = torch.randn(2 * K if glu else K, device=dev, dtype=torch.float16, generator=g)
        res = torch.randn(N, device=dev, dtype=torch.float16, generator=g)
        forms = {"native": lambda i: ops.gemv_fused(ws[i % ncopy], x, None, glu=glu, residual=res),
                 "e4m3": lambda i: w8.gemv_w8(*packs[i % ncopy], x, None, glu=glu, residual=res)}
        out = {}
        for mode, fn in forms.items():
            for i in range(3):
                fn(i)
            best = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(iters):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                best.append(e0.elapsed_time(e1) * 1e3 / iters)
            us = sorted(best)[len(best) // 2]
            out[mode] = (us, N * K * (2 if mode == "native" else 1) / us * 1e-3)
        log(f"{name:<10} {N:>7} {K:>6} | {out['native'][0]:>10.1f} {out['native'][1]:>7.0f} | {out['e4m3'][0]:>9.1f} {out['e4m3'][1]:>7.0f} | "
            f"{out['e4m3'][0] / out['native'][0]:.3f}")
        del ws, packs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=256)
    ap.add_argument("--forced_steps", type=int, default=64)
    ap.add_argument("--gemv_only", action="store_true", help="only the per-shape GEMV rates (no model is built)")
    a = ap.parse_args(argv)
    if a.gemv_only:
        gemv_rates(torch.device("cuda:0"), print)
        return
    from rsvld_amd import llava_next as LN
    from tools import synthetic_models as SM
    dev = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# caption token loop, native vs e4m3 weights: {torch.cuda.get_device_name(0)}, 8 B decoder (seeded), prompt {a.prompt}, "
        f"{a.new_tokens} greedy tokens")
    model = SM.llava_full(dev)[0]
    ids = torch.randint(1000, 100000, (1, a.prompt), generator=torch.Generator().manual_seed(7)).to(dev)
    max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
    with torch.no_grad():
        emb = model.model.embed_tokens(ids)
        dec = {"e4m3": LN.FastDecoder(model, max_len, weights="e4m3"), "native": LN.FastDecoder(model, max_len)}
        toks = {}
        for mode in ("native", "e4m3"):      # warm-up: allocator, graph capture
            toks[mode] = dec[mode].generate(emb, a.new_tokens, do_sample=False)
        log("\n## ms per token (FastDecoder.profile: the loop behind the prefill, sampling included)")
        pairs = []
        for order in (("native", "e4m3"), ("native", "e4m3"), ("e4m3", "native"), ("e4m3", "native")):
            ms = {}
            for mode in order:
                dec[mode].profile = {}
                dec[mode].generate(emb, a.new_tokens, do_sample=False)
                p = dec[mode].profile
                ms[mode] = p["decode_s"] * 1e3 / max(1, p["new_tokens"] - 1)
                dec[mode].profile = None
            pairs.append(ms)
            log(f"pair {len(pairs)} ({order[0]} first): native {ms['native']:.3f} ms/token, e4m3 {ms['e4m3']:.3f} ms/token, "
                f"e4m3 / native = {ms['e4m3'] / ms['native']:.3f}")
        log(f"e4m3 faster in every pair: {all(p['e4m3'] < p['native'] for p in pairs)}")
        log("\n## teacher forcing on the native loop's greedy tokens")
        T0 = a.prompt
        lg = {}
        for mode in ("native", "e4m3"):
            d = dec[mode]
            out = [d.forward(emb.to(d.dt), torch.arange(T0, device=dev)).float()]
            for n in range(a.forced_steps):
                out.append(d.forward(model.model.embed_tokens(toks["native"][n].view(1))[None], torch.tensor([T0 + n], device=dev)).float())
            lg[mode] = torch.cat(out)[1:]
        rel = (lg["e4m3"] - lg["native"]).abs().amax(1) / lg["native"].abs().amax(1)
        agree = (lg["e4m3"].argmax(1) == lg["native"].argmax(1)).float().mean()
        log(f"{a.forced_steps} steps: max|logits_e4m3 - logits_native| / max|logits_native| = mean {float(rel.mean()):.4f}, worst {float(rel.max()):.4f}; "
            f"top-1 agreement {float(agree):.3f}")
        log(f"free-running greedy loops agree on the first {int((toks['native'] != toks['e4m3']).float().cumsum(0).eq(0).sum())} of {a.new_tokens} tokens")
        del dec, lg
        log("\n## weight bytes per second, per GEMV shape (fp16 activations; fused form of the layer: down_proj with SwiGLU, all with the residual)")
        gemv_rates(dev, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
