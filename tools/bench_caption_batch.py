"""A-B of the caption pass's token loop one caption at a time (``FastDecoder.generate``, the loop ``infer_dir`` runs per image) against the
batched loop (``FastDecoder.generate_batch``, ``--caption_batch B``) at B = 1, 2, 4, 8, for the 16-bit weights and the e4m3 ones, in ONE
process on one device: the full-size seeded 8 B decoder of tools/synthetic_models.py, 256 greedy tokens behind prompts of the bench's
length (3 047 positions: profiles/r06_bench_c4.json).

  * token loop: ms per step and ms per step and row from ``FastDecoder.profile`` (device-synchronised wall time of the loop behind the
    prefills, sampling included), single and batched alternating -- S B S B S B, then B S B S B S: six pairs, three in each order -- and
    from them the token-loop seconds per image at group size B against the single loop of the same run;
  * per GEMV shape of the decoder and B: us per launch and GB/s of weight bytes, over weight copies that rotate through more memory than
    the 256 MB last-level cache holds, and whether the launch still takes the single-row kernel's time (i.e. is still bound by the
    weight bytes) or is bound by the per-row arithmetic.

The batched results are the single ones bit for bit (tests/test_gpu_decode_rows.py); the greedy tokens are compared here once more.

    python tools/bench_caption_batch.py --out profiles/caption_batch_ab.txt
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
BATCHES = (1, 2, 4, 8)
BOUND = 1.15      # a multi-row launch within this factor of the single-row kernel's time counts as still bound by the weight bytes


def _time(fn, iters, repeats):
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
    return sorted(best)[len(best) // 2]


def gemv_rates(dev, log, iters=20, repeats=5):
    from rsvld_amd import decode_rows as DR, ops, w8
    log(f"{'shape':<10} {'N':>7} {'K':>6} {'weights':>7} | {'single us':>9} {'GB/s':>6} | " +
        " | ".join(f"B={B} us {'GB/s':>6} {'bound':>7}" for B in BATCHES))
    g = torch.Generator(device=dev).manual_seed(1)
    for name, N, K in SHAPES:
        ncopy = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        ws = [torch.empty(N, K, device=dev, dtype=torch.float16).normal_(0, 0.02, generator=g) for _ in range(ncopy)]
        packs = [w8.pack_rows_e4m3(w) for w in ws]
        glu = name == "down_proj"
        x = torch.randn(8, 2 * K if glu else K, device=dev, dtype=torch.float16, generator=g)
        res = torch.randn(8, N, device=dev, dtype=torch.float16, generator=g)
        for mode, nbytes in (("native", N * K * 2), ("e4m3", N * K)):
            if mode == "native":
                single = lambda i: ops.gemv_fused(ws[i % ncopy], x[0], None, glu=glu, residual=res[0])
                rows = lambda B: (lambda i: DR.gemv_rows(ws[i % ncopy], x[:B], None, glu=glu, residual=res[:B]))
            else:
                single = lambda i: w8.gemv_w8(*packs[i % ncopy], x[0], None, glu=glu, residual=res[0])
                rows = lambda B: (lambda i: DR.gemv_w8_rows(*packs[i % ncopy], x[:B], None, glu=glu, residual=res[:B]))
            us1 = _time(single, iters, repeats)
            cells = []
            for B in BATCHES:
                us = _time(rows(B), iters, repeats)
                cells.append(f"{us:>8.1f} {nbytes / us * 1e-3:>6.0f} {'weights' if us <= BOUND * us1 else 'rows':>7}")
            log(f"{name:<10} {N:>7} {K:>6} {mode:>7} | {us1:>9.1f} {nbytes / us1 * 1e-3:>6.0f} | " + " | ".join(cells))
        del ws, packs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=3, help="pairs per order (>= 3 in all)")
    ap.add_argument("--gemv_only", action="store_true", help="only the per-shape GEMV rates (no model is built)")
    a = ap.parse_args(argv)
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

    log(f"# caption token loop, one caption at a time vs B captions per loop: {torch.cuda.get_device_name(0)}, 8 B decoder (seeded), "
        f"prompt {a.prompt}, {a.new_tokens} greedy tokens")
    if not a.gemv_only:
        from rsvld_amd import llava_next as LN
        from tools import synthetic_models as SM
        model = SM.llava_full(dev)[0]
        max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
        with torch.no_grad():
            embs = [model.model.embed_tokens(torch.randint(1000, 100000, (1, a.prompt), generator=torch.Generator().manual_seed(7 + b)).to(dev))
                    for b in range(max(BATCHES))]
            for mode in ("native", "e4m3"):
                log(f"\n## weights = {mode}: ms per step of the token loop (FastDecoder.profile: the loop behind the prefills, sampling included)")
                dec = LN.FastDecoder(model, max_len, weights=mode, batch=max(BATCHES))

                def single():
                    dec.profile = {}
                    t = dec.generate(embs[0], a.new_tokens, do_sample=False)
                    p, dec.profile = dec.profile, None
                    return p["decode_s"] * 1e3 / max(1, p["new_tokens"] - 1), t

                def batched(B):
                    dec.profile = {}
                    t = dec.generate_batch(embs[:B], a.new_tokens, do_sample=False)
                    p, dec.profile = dec.profile, None
                    return p["decode_s"] * 1e3 / max(1, p["steps"]), t

                want = single()[1]                                  # warm-up: allocator, graph capture
                summary = []
                for B in BATCHES:
                    same = torch.equal(batched(B)[1][0], want)      # warm-up of this B; row 0 is the single loop's prompt
                    s_ms, b_ms = [], []
                    for order in ("SB",) * a.pairs + ("BS",) * a.pairs:
                        ms = {}
                        for which in order:
                            ms[which] = single()[0] if which == "S" else batched(B)[0]
                        s_ms.append(ms["S"])
                        b_ms.append(ms["B"])
                        log(f"B={B} pair {len(s_ms)} ({'single' if order[0] == 'S' else 'batched'} first): single {ms['S']:.3f} ms/step, "
                            f"batched {ms['B']:.3f} ms/step = {ms['B'] / B:.3f} ms/step and row, per row / single = {ms['B'] / B / ms['S']:.3f}")
                    s_med, b_med = sorted(s_ms)[len(s_ms) // 2], sorted(b_ms)[len(b_ms) // 2]
                    summary.append((B, s_med, b_med, same, all(b / B < s for s, b in zip(s_ms, b_ms))))
                n = a.new_tokens - 1
                log(f"\n{'B':>2} | {'ms/step':>8} {'ms/step/row':>11} | token loop s/image | single loop s/image | saved s/image | row 0 == single | "
                    f"faster per row in every pair")
                for B, s_med, b_med, same, faster in summary:
                    log(f"{B:>2} | {b_med:>8.3f} {b_med / B:>11.3f} | {b_med / B * n * 1e-3:>18.3f} | {s_med * n * 1e-3:>19.3f} | "
                        f"{(s_med - b_med / B) * n * 1e-3:>13.3f} | {str(same):>15} | {faster}")
                save()
                del dec
                model.__dict__.pop("_fast_decoder", None)
        del model, embs
        torch.cuda.empty_cache()
    log("\n## per GEMV shape: us per launch and GB/s of weight bytes (fp16 activations; fused form of the layer: down_proj with SwiGLU, all "
        f"with the residual); bound = weights: within {BOUND} x the single-row kernel's time, rows: slower (the per-row arithmetic binds)")
    gemv_rates(dev, log)
    save()


if __name__ == "__main__":
    main()
