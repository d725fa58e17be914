"""What the e4m3-only caption mode costs and frees (``FastDecoder(weights="e4m3", prefill_weights="e4m3", release_native=True)``,
``--caption_weights e4m3-only``; csrc/gemm_w8.hip), in ONE process on one device: the full-size seeded 8 B decoder of
tools/synthetic_models.py behind a prompt of the bench's length (3 047 positions), cache length 3 328.

  * per shape: us and TFLOP/s of ``w8.linear_w8`` against ``torch.nn.functional.linear`` on the 16-bit tensor, M = prompt rows, the four
    (N, K) of a decoder layer (device events around batches of launches);
  * memory: ``torch.cuda.memory_allocated`` with the decoder built -- native, e4m3, and e4m3 released -- and the peak while the released
    one is built (from an emptied allocator cache);
  * prefill: ``FastDecoder.profile["prefill_s"]`` of ``weights="e4m3"`` with the 16-bit prefill (the behaviour without this mode) against
    ``prefill_weights="e4m3"``, both attention routes, the two alternating -- A B x 3, then B A x 3 -- per pair and as medians.  ONE decoder
    per attention route serves both sides: ``prefill_weights`` is read by ``forward`` alone, so the A side is that decoder with the field
    set to "native" (same packs, same cache, same 16-bit tensors);
  * token loop: ``decode_s`` per generated token of the released decoder beside the e4m3 one (the same captured step on the same packs).

The released decoder is built LAST: it empties the model.  There is no threshold here: the numbers are written down, not met.

    python tools/bench_caption_e4m3_only.py --out profiles/caption_e4m3_only_ab.txt
"""
import argparse
import dataclasses
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("q|k|v", 6144, 4096), ("o_proj", 4096, 4096), ("gate|up", 28672, 4096), ("down_proj", 4096, 14336)]


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


def per_shape(dev, log, M, iters=10, repeats=5):
    """-> (sum of the four medians of linear_w8, of F.linear) in us: one layer's projections."""
    from rsvld_amd import w8
    gen = torch.Generator(device=dev).manual_seed(3)
    tot8 = tot16 = 0.0
    for name, N, K in SHAPES:
        w = (torch.randn(N, K, device=dev, dtype=torch.float32, generator=gen) / K ** 0.5).half()
        x = torch.randn(M, K, device=dev, dtype=torch.float16, generator=gen)
        q, scale = w8.pack_rows_e4m3(w)
        pl = w8.plan_linear(M, N, K)
        flops = 2.0 * M * N * K
        m8, lo8, hi8 = _time_us(lambda: w8.linear_w8(q, scale, x), iters, repeats)
        m16, lo16, hi16 = _time_us(lambda: torch.nn.functional.linear(x, w), iters, repeats)
        tot8, tot16 = tot8 + m8, tot16 + m16
        log(f"{name:9s} N {N:6d} K {K:6d}: linear_w8 {m8:8.1f} us (min {lo8:.1f}, max {hi8:.1f}) = {flops / m8 * 1e-6:6.1f} TFLOP/s, grid "
            f"{pl.grid_x} x {pl.grid_y} | F.linear fp16 {m16:8.1f} us (min {lo16:.1f}, max {hi16:.1f}) = {flops / m16 * 1e-6:6.1f} TFLOP/s | "
            f"linear_w8 / F.linear = {m8 / m16:.2f}")
        del w, x, q, scale
    log(f"one layer's four projections: linear_w8 {tot8:.1f} us, F.linear {tot16:.1f} us; 32 layers: {32 * tot8 * 1e-3:.2f} ms vs "
        f"{32 * tot16 * 1e-3:.2f} ms ({repeats} batches of {iters} launches each)")
    return tot8, tot16


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=256, help="sizes the cache (prompt + new tokens, rounded up to 256)")
    ap.add_argument("--loop_tokens", type=int, default=64, help="tokens of the timed token loop")
    ap.add_argument("--pairs", type=int, default=3, help="pairs per order (>= 3 in all)")
    ap.add_argument("--kernel_only", action="store_true", help="only the per-shape table (no model is built)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_caption_e4m3_only: no GPU visible (a measurement needs one; there is no CPU stand-in)")
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

    gib = lambda b: b / 2 ** 30
    max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
    log(f"# caption on e4m3 weights alone (prefill_weights='e4m3', release_native): {torch.cuda.get_device_name(0)}, 8 B decoder (seeded, "
        f"fp16), prompt {a.prompt}, cache length {max_len}")
    log(f"\n## the projections of one layer at M = {a.prompt} rows: w8.linear_w8 (e4m3 bytes, rsvld_gemm_w8) vs F.linear on the fp16 tensor; device events")
    per_shape(dev, log, a.prompt)
    save()
    if a.kernel_only:
        return
    from rsvld_amd import llava_next as LN
    from tools import synthetic_models as SM
    model = SM.llava_full(dev)[0]
    alloc = lambda: torch.cuda.memory_allocated(dev)

    def settle():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    with torch.no_grad():
        emb = model.model.embed_tokens(torch.randint(1000, 100000, (1, a.prompt), generator=torch.Generator().manual_seed(7)).to(dev))
        settle()
        m_model = alloc()
        log(f"\n## memory (torch.cuda.memory_allocated, GiB): the model alone (decoder, vision tower, projector) {gib(m_model):.2f}")
        dec = LN.FastDecoder(model, max_len)
        settle()
        m_native = alloc()
        del dec
        settle()

        def loop_ms(dec):
            """-> median ms per token of ``decode_s`` over three runs of the captured loop (after one run that captures it)."""
            out = []
            for i in range(4):
                dec.profile = {}
                dec.generate(emb, a.loop_tokens, do_sample=False)
                p, dec.profile = dec.profile, None
                if i:
                    out.append(p["decode_s"] * 1e3 / (p["new_tokens"] - 1))
            return _median(out), min(out), max(out)

        def prefill(dec, pw):
            dec.mode = dataclasses.replace(dec.mode, prefill_weights=pw)
            dec.profile = {}
            tok = dec.generate(emb, 1, do_sample=False, use_graph=False)
            p, dec.profile = dec.profile, None
            return p["prefill_s"] * 1e3, tok

        m_e4m3 = None
        for route in ("flash", "torch"):
            dec = LN.FastDecoder(model, max_len, weights="e4m3", prefill=route, prefill_weights="e4m3")
            if m_e4m3 is None:
                settle()
                m_e4m3 = alloc()
                loop_e4m3 = loop_ms(dec)
            for pw in ("native", "e4m3"):                          # warm-up: allocator, library algorithm choices, code objects
                prefill(dec, pw)
                prefill(dec, pw)
            dec.mode = dataclasses.replace(dec.mode, prefill_weights="native")
            l16 = dec.forward(emb.to(torch.float16), torch.arange(a.prompt, device=dev), pos0=0).float()
            dec.mode = dataclasses.replace(dec.mode, prefill_weights="e4m3")
            l8 = dec.forward(emb.to(torch.float16), torch.arange(a.prompt, device=dev), pos0=0).float()
            log(f"\n## prefill, attention route '{route}': prefill_s of weights='e4m3' with the 16-bit prefill (A) vs prefill_weights='e4m3' (B), alternating pairs")
            log(f"prefill logits: max |B - A| = {float((l8 - l16).abs().max()):.3e} (max |A| = {float(l16.abs().max()):.3e}); argmax equal: "
                f"{bool(l8.argmax() == l16.argmax())}  (two models: A's prompt is read by the 16-bit weights, B's by dequant(pack(w)))")
            ms = {"native": [], "e4m3": []}
            for n, order in enumerate((("native", "e4m3"),) * a.pairs + (("e4m3", "native"),) * a.pairs):
                got = {}
                for pw in order:
                    got[pw] = prefill(dec, pw)[0]
                    ms[pw].append(got[pw])
                log(f"pair {n + 1} ({'A' if order[0] == 'native' else 'B'} first): A 16-bit {got['native']:8.2f} ms | B e4m3 {got['e4m3']:8.2f} ms | "
                    f"B / A = {got['e4m3'] / got['native']:.3f}")
            ma, mb = _median(ms["native"]), _median(ms["e4m3"])
            log(f"median prefill ({route}): A 16-bit {ma:.2f} ms, B e4m3 {mb:.2f} ms, B / A = {mb / ma:.3f} ({mb - ma:+.2f} ms); B faster in "
                f"{sum(b < x for b, x in zip(ms['e4m3'], ms['native']))} of {len(ms['native'])} pairs")
            save()
            del dec
            settle()
        # ---- the released decoder, last: it empties the model
        base = alloc()
        torch.cuda.reset_peak_memory_stats(dev)
        dec = LN.FastDecoder(model, max_len, weights="e4m3", prefill="flash", prefill_weights="e4m3", release_native=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
        settle()
        m_rel = alloc()
        loop_rel = loop_ms(dec)
        log(f"\n## memory with the decoder built (GiB; cache length {max_len}, one row)")
        log(f"native                       {gib(m_native):7.2f}")
        log(f"e4m3 (packs beside 16-bit)   {gib(m_e4m3):7.2f}   ({gib(m_e4m3 - m_native):+.2f} against native)")
        log(f"e4m3 released                {gib(m_rel):7.2f}   ({gib(m_rel - m_native):+.2f} against native, {gib(m_rel - m_e4m3):+.2f} against e4m3)")
        log(f"peak while the released decoder was built: {gib(peak):.2f} = {gib(peak - base):+.3f} above the {gib(base):.2f} allocated before it")
        log(f"\n## token loop, ms per token (decode_s / (new tokens - 1), {a.loop_tokens} tokens, median of 3 runs of the captured loop; min, max)")
        log(f"e4m3           {loop_e4m3[0]:.3f}  ({loop_e4m3[1]:.3f}, {loop_e4m3[2]:.3f})")
        log(f"e4m3 released  {loop_rel[0]:.3f}  ({loop_rel[1]:.3f}, {loop_rel[2]:.3f})   released / e4m3 = {loop_rel[0] / loop_e4m3[0]:.3f}")
    save()


if __name__ == "__main__":
    main()
