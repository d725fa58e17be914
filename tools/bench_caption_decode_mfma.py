"""A-B of the caption pass's token loop on the VALU products (``FastDecoder(decode="valu")``, csrc/gemv.hip) against the MFMA products
(``decode="mfma"``, csrc/gemv_mma.hip) at B = 1, 2, 4, 8 captions per loop, for the 16-bit weights and the e4m3 ones, in ONE process on
one device: the full-size seeded 8 B decoder of tools/synthetic_models.py behind prompts of the bench's length (3 047 positions:
profiles/r06_bench_c4.json).

  * token loop: ms per step from ``FastDecoder.profile`` (device-synchronised wall time of the loop behind the prefills, sampling
    included; B = 1: ``generate``, B > 1: ``generate_batch``), the two modes alternating -- V M V M V M, then M V M V M V: six pairs,
    three in each order -- the median per mode, their ratio, and in how many pairs each mode was the faster one;
  * per product shape of the decoder, at B = 1, 4, 8: us per launch and TB/s of weight bytes of both kernels, over weight copies that
    rotate through more memory than the 256 MB last-level cache holds; and the cost of down_proj's second weight pass at B = 8 (its
    eight staged rows exceed the LDS: two groups of four);
  * ``--resources`` (no GPU needed): the compiler's resource report of csrc/gemv_mma.hip.

Inside the MFMA mode a batched caption is the single caption token for token (tests/test_gpu_caption_decode_mfma.py); row 0 is compared
here once more.

    python tools/bench_caption_decode_mfma.py --out profiles/caption_decode_mfma_ab.txt
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("q|k|v", 6144, 4096), ("o_proj", 4096, 4096), ("gate|up", 28672, 4096), ("down_proj", 4096, 14336), ("lm_head", 128256, 4096)]
ROTATE_BYTES = 2 << 30
BATCHES = (1, 2, 4, 8)
SHAPE_ROWS = (1, 4, 8)
MODES = ("valu", "mfma")


def _time(fn, iters, repeats):
    import torch
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
    import torch
    from rsvld_amd import decode_rows as DR, w8
    log(f"{'shape':<10} {'N':>7} {'K':>6} {'weights':>7} | " + " | ".join(f"B={B}: valu us TB/s   mfma us TB/s  mfma/valu" for B in SHAPE_ROWS))
    g = torch.Generator(device=dev).manual_seed(1)
    second_pass = []
    for name, N, K in SHAPES:
        ncopy = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        ws = [torch.empty(N, K, device=dev, dtype=torch.float16).normal_(0, 0.02, generator=g) for _ in range(ncopy)]
        packs = [w8.pack_rows_e4m3(w) for w in ws]
        glu = name == "down_proj"
        x = torch.randn(8, 2 * K if glu else K, device=dev, dtype=torch.float16, generator=g)
        res = torch.randn(8, N, device=dev, dtype=torch.float16, generator=g)
        for weights, nbytes in (("native", N * K * 2), ("e4m3", N * K)):
            if weights == "native":
                rows = lambda B, k: (lambda i: DR.gemv_rows(ws[i % ncopy], x[:B], None, glu=glu, residual=res[:B], kernel=k))
            else:
                rows = lambda B, k: (lambda i: DR.gemv_w8_rows(*packs[i % ncopy], x[:B], None, glu=glu, residual=res[:B], kernel=k))
            cells, us_m = [], {}
            for B in SHAPE_ROWS:
                us = {k: _time(rows(B, k), iters, repeats) for k in MODES}
                us_m[B] = us["mfma"]
                cells.append(f"     {us['valu']:>8.1f} {nbytes / us['valu'] * 1e-6:>4.2f} {us['mfma']:>9.1f} {nbytes / us['mfma'] * 1e-6:>4.2f} "
                             f"{us['mfma'] / us['valu']:>10.3f}")
            log(f"{name:<10} {N:>7} {K:>6} {weights:>7} | " + " | ".join(cells))
            if glu:
                second_pass.append(f"down_proj {weights}: mfma B=4 (one weight pass) {us_m[4]:.1f} us, B=8 (two groups of four, two passes) "
                                   f"{us_m[8]:.1f} us: the second pass costs {us_m[8] - us_m[4]:.1f} us per step and layer")
        del ws, packs
    log("")
    for s in second_pass:
        log(s)


def resources(log):
    """The compiler's report of csrc/gemv_mma.hip (hipcc -Rpass-analysis=kernel-resource-usage), one line per kernel."""
    src = os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", f"-I{src}",
               f"-I{os.path.join(ROOT, 'include')}", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-o", os.path.join(tmp, "unit.s"), os.path.join(src, "gemv_mma.hip")]
        err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    log("\n## compiler report of csrc/gemv_mma.hip (gfx950; kernel<T, KSPLIT, W8>; LDS is dynamic: staged rows + 32 KiB of slabs (+ 4 KiB of partial sums))")
    cur = {}
    for line in err.splitlines():
        m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            t = re.search(r"gemv_mma_kernelI(DF16_|DF16b)Lb([01])ELb([01])E", cur["name"])
            tag = f"<{'f16' if t.group(1) == 'DF16_' else 'bf16'}, KSPLIT={t.group(2)}, W8={t.group(3)}>" if t else cur["name"]
            log(f"gemv_mma_kernel{tag}: VGPRs {cur['VGPRs']}, AGPRs {cur['AGPRs']}, scratch {cur['ScratchSize [bytes/lane]']} bytes/lane, "
                f"occupancy {cur['Occupancy [waves/SIMD]']} waves/SIMD, static LDS {cur['LDS Size [bytes/block]']}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3, help="pairs per order (>= 3 in all)")
    ap.add_argument("--gemv_only", action="store_true", help="only the per-shape rates (no model is built)")
    ap.add_argument("--resources", action="store_true", help="only the compiler report (no GPU needed)")
    a = ap.parse_args(argv)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.resources:
        resources(log)
        save()
        return
    import torch
    dev = torch.device("cuda:0")
    log(f"# caption token loop, decode=valu vs decode=mfma: {torch.cuda.get_device_name(0)}, 8 B decoder (seeded), prompt {a.prompt}, "
        f"{a.new_tokens} greedy tokens")
    if not a.gemv_only:
        from rsvld_amd import llava_next as LN
        from tools import synthetic_models as SM
        model = SM.llava_full(dev)[0]
        max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
        with torch.no_grad():
            embs = [model.model.embed_tokens(torch.randint(1000, 100000, (1, a.prompt), generator=torch.Generator().manual_seed(7 + b)).to(dev))
                    for b in range(max(BATCHES))]
            for weights in ("native", "e4m3"):
                log(f"\n## weights = {weights}: ms per step of the token loop (FastDecoder.profile: the loop behind the prefills, sampling included)")
                decs = {k: LN.FastDecoder(model, max_len, weights=weights, batch=max(BATCHES), decode=k) for k in MODES}

                def run(k, B):
                    dec = decs[k]
                    dec.profile = {}
                    if B == 1:
                        t = [dec.generate(embs[0], a.new_tokens, do_sample=False)]
                        steps = dec.profile["new_tokens"] - 1
                    else:
                        t = dec.generate_batch(embs[:B], a.new_tokens, do_sample=False)
                        steps = dec.profile["steps"]
                    p, dec.profile = dec.profile, None
                    return p["decode_s"] * 1e3 / max(1, steps), t

                single = run("mfma", 1)[1][0]
                summary = []
                for B in BATCHES:
                    same = all(torch.equal(run(k, B)[1][0], single if k == "mfma" else run("valu", 1)[1][0]) for k in MODES)   # warm-up too
                    ms = {k: [] for k in MODES}
                    for order in (MODES,) * a.pairs + (MODES[::-1],) * a.pairs:
                        for k in order:
                            ms[k].append(run(k, B)[0])
                        log(f"B={B} pair {len(ms['valu'])} ({order[0]} first): valu {ms['valu'][-1]:.3f} ms/step, mfma {ms['mfma'][-1]:.3f} ms/step, "
                            f"mfma / valu = {ms['mfma'][-1] / ms['valu'][-1]:.3f}")
                    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
                    wins = sum(m < v for v, m in zip(ms["valu"], ms["mfma"]))
                    summary.append((B, med, wins, len(ms["valu"]) - wins, same))
                log(f"\n{'B':>2} | {'valu ms/step':>12} {'mfma ms/step':>12} {'mfma / valu':>11} | {'mfma ms/step/row':>16} | mfma faster in | valu faster in | "
                    f"row 0 == the mode's single loop")
                for B, med, wins, losses, same in summary:
                    log(f"{B:>2} | {med['valu']:>12.3f} {med['mfma']:>12.3f} {med['mfma'] / med['valu']:>11.3f} | {med['mfma'] / B:>16.3f} | "
                        f"{wins:>8} pairs | {losses:>8} pairs | {same}")
                save()
                del decs
                model.__dict__.pop("_fast_decoder", None)
                torch.cuda.empty_cache()
        del model, embs
        torch.cuda.empty_cache()
    log("\n## per product shape: us per launch and TB/s of weight bytes (fp16 activations; fused form of the layer: down_proj with SwiGLU, all "
        "with the residual)")
    gemv_rates(dev, log)
    save()


if __name__ == "__main__":
    main()
