"""A-B of the token loop's decode attention: the VALU operator (da_kernel + da_combine_kernel of csrc/decode_attention.hip) against the MFMA
operator (dam_prologue_kernel + dam_kernel + da_combine_kernel of the same unit, ``FastDecoder(decode_attention="mfma")``) at B = 1, 2, 4, 8
sequences, in ONE process on one device, on the shape of the full-size seeded 8 B decoder of tools/synthetic_models.py: 32 query heads
on 8 kv heads, max_len 3 328, positions from 3 047 (the bench's prompt: profiles/r06_bench_c4.json).  The protocol of
tools/bench_caption_decode_mfma.py: six alternated pairs per cell, three in each order, the median per mode.

  (a) ``--launches``: us per call of either operator (all its launches: 2 / 3) by HIP events around replays of a hipGraph that holds
      one pass over 32 pairs of caches -- the decoder's 32 layers, more memory than the 256 MB last-level cache holds, replayed as the
      token loop replays its step -- fp16; beside each the key / value bytes the call has to read and the TB/s they imply;
  (b) ``--loop``: ms per step of the token loop (``FastDecoder.profile``, ``decode="mfma"``) for the 16-bit and the e4m3 weights,
      ``decode_attention`` valu against mfma, and whether row 0 of the batched loop equals the mode's single loop;
  ``--resources`` (no GPU needed): the compiler's resource report of csrc/decode_attention.hip.

    python tools/bench_caption_decode_attention.py --launches --loop --resources --out profiles/caption_decode_attention_ab.txt
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

N_Q, N_KV, HD, LAYERS = 32, 8, 128, 32
BATCHES = (1, 2, 4, 8)
MODES = ("valu", "mfma")


def _median(v):
    return sorted(v)[len(v) // 2]


def launches(dev, log, max_len, pos0, pairs, iters=LAYERS * 8):
    import torch
    from rsvld_amd import decode_rows as DR, ops
    dt = torch.float16
    g = torch.Generator(device=dev).manual_seed(3)
    B8 = max(BATCHES)
    caches = [(torch.empty(B8, N_KV, max_len, HD, device=dev, dtype=dt).normal_(0, 1, generator=g),
               torch.empty(B8, N_KV, max_len, HD, device=dev, dtype=dt).normal_(0, 1, generator=g)) for _ in range(LAYERS)]
    qkv = torch.randn(B8, (N_Q + 2 * N_KV) * HD, device=dev, dtype=dt, generator=g)
    ang = torch.rand(B8, HD // 2, device=dev, generator=g) * 6
    cos, sin = torch.cat([ang.cos(), ang.cos()], dim=1).to(dt), torch.cat([ang.sin(), ang.sin()], dim=1).to(dt)
    ws = {k: torch.empty(DR.decode_attention_ws_floats(N_Q, N_KV, max_len, B8, k), device=dev) for k in MODES}
    log(f"\n## (a) us per call of the operator (all its launches), fp16, {N_Q} heads on {N_KV}, max_len {max_len}, positions {pos0} + b, "
        f"{LAYERS} cache pairs in one replayed hipGraph; K/V bytes = 2 x B x {N_KV} x (pos + 1) x {HD} x 2 B")
    summary = []
    for B in BATCHES:
        pos = torch.arange(pos0, pos0 + B, device=dev)
        nbytes = sum(2 * N_KV * (pos0 + b + 1) * HD * 2 for b in range(B))

        graphs = {}
        for k in MODES:      # one pass over the layers, captured: the token loop replays its step from a hipGraph, so the host's launch rate is no part of it
            def layers():
                for kc, vc in caches:
                    DR.llama_decode_attention_rows(qkv[:B], cos[:B], sin[:B], pos, kc[:B], vc[:B], N_Q, N_KV, HD ** -0.5, ws=ws[k], kernel=k)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                layers()
            torch.cuda.current_stream().wait_stream(side)
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                layers()

        def run(k):
            graphs[k].replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters // LAYERS):
                graphs[k].replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (iters // LAYERS * LAYERS)

        us = {k: [] for k in MODES}
        for order in (MODES,) * pairs + (MODES[::-1],) * pairs:
            for k in order:
                us[k].append(run(k))
            log(f"B={B} pair {len(us['valu'])} ({order[0]} first): valu {us['valu'][-1]:.1f} us, mfma {us['mfma'][-1]:.1f} us, "
                f"mfma / valu = {us['mfma'][-1] / us['valu'][-1]:.3f}")
        med = {k: _median(v) for k, v in us.items()}
        wins = sum(m < v for v, m in zip(us["valu"], us["mfma"]))
        summary.append((B, nbytes, med, wins, len(us["valu"]) - wins))
    log(f"\n{'B':>2} | {'K/V MB':>7} | {'valu us':>8} {'TB/s':>5} | {'mfma us':>8} {'TB/s':>5} | {'mfma / valu':>11} | mfma faster in | valu faster in | "
        f"x {LAYERS} layers: valu ms, mfma ms")
    for B, nbytes, med, wins, losses in summary:
        log(f"{B:>2} | {nbytes / 1e6:>7.1f} | {med['valu']:>8.1f} {nbytes / med['valu'] * 1e-6:>5.2f} | {med['mfma']:>8.1f} "
            f"{nbytes / med['mfma'] * 1e-6:>5.2f} | {med['mfma'] / med['valu']:>11.3f} | {wins:>8} pairs | {losses:>8} pairs | "
            f"{med['valu'] * LAYERS * 1e-3:.3f}, {med['mfma'] * LAYERS * 1e-3:.3f}")


def loop(dev, log, save, prompt, new_tokens, pairs):
    import torch
    from rsvld_amd import llava_next as LN
    from tools import synthetic_models as SM
    model = SM.llava_full(dev)[0]
    max_len = -(-(prompt + new_tokens) // 256) * 256
    with torch.no_grad():
        embs = [model.model.embed_tokens(torch.randint(1000, 100000, (1, prompt), generator=torch.Generator().manual_seed(7 + b)).to(dev))
                for b in range(max(BATCHES))]
        for weights in ("native", "e4m3"):
            log(f"\n## (b) weights = {weights}, decode = mfma: ms per step of the token loop (FastDecoder.profile: the loop behind the prefills, "
                f"sampling included), prompt {prompt}, {new_tokens} greedy tokens, max_len {max_len}")
            decs = {k: LN.FastDecoder(model, max_len, weights=weights, batch=max(BATCHES), decode="mfma", decode_attention=k) for k in MODES}

            def run(k, B):
                dec = decs[k]
                dec.profile = {}
                if B == 1:
                    t = [dec.generate(embs[0], new_tokens, do_sample=False)]
                    steps = dec.profile["new_tokens"] - 1
                else:
                    t = dec.generate_batch(embs[:B], new_tokens, do_sample=False)
                    steps = dec.profile["steps"]
                p, dec.profile = dec.profile, None
                return p["decode_s"] * 1e3 / max(1, steps), t

            single = {k: run(k, 1)[1][0] for k in MODES}
            summary = []
            for B in BATCHES:
                same = all(torch.equal(run(k, B)[1][0], single[k]) for k in MODES)      # (the warm-up of the cell too)
                ms = {k: [] for k in MODES}
                for order in (MODES,) * pairs + (MODES[::-1],) * pairs:
                    for k in order:
                        ms[k].append(run(k, B)[0])
                    log(f"B={B} pair {len(ms['valu'])} ({order[0]} first): valu {ms['valu'][-1]:.3f} ms/step, mfma {ms['mfma'][-1]:.3f} ms/step, "
                        f"mfma / valu = {ms['mfma'][-1] / ms['valu'][-1]:.3f}")
                med = {k: _median(v) for k, v in ms.items()}
                wins = sum(m < v for v, m in zip(ms["valu"], ms["mfma"]))
                summary.append((B, med, wins, len(ms["valu"]) - wins, same))
            log(f"\n{'B':>2} | {'valu ms/step':>12} {'mfma ms/step':>12} {'mfma / valu':>11} | mfma faster in | valu faster in | "
                f"row 0 == the mode's single loop")
            for B, med, wins, losses, same in summary:
                log(f"{B:>2} | {med['valu']:>12.3f} {med['mfma']:>12.3f} {med['mfma'] / med['valu']:>11.3f} | {wins:>8} pairs | {losses:>8} pairs | {same}")
            save()
            del decs
            torch.cuda.empty_cache()


def resources(log):
    """The compiler's report of csrc/decode_attention.hip (hipcc -Rpass-analysis=kernel-resource-usage), one line per kernel."""
    src = os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", f"-I{src}",
               f"-I{os.path.join(ROOT, 'include')}", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-o", os.path.join(tmp, "unit.s"), os.path.join(src, "decode_attention.hip")]
        err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    log("\n## compiler report of csrc/decode_attention.hip (gfx950)")
    cur = {}
    for line in err.splitlines():
        m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            t = re.search(r"(dam_prologue_kernel|dam_kernel)I(DF16_|DF16b)", cur["name"])
            tag = f"{t.group(1)}<{'f16' if t.group(2) == 'DF16_' else 'bf16'}>" if t else cur["name"]
            log(f"{tag}: VGPRs {cur['VGPRs']}, AGPRs {cur['AGPRs']}, scratch {cur['ScratchSize [bytes/lane]']} bytes/lane, "
                f"occupancy {cur['Occupancy [waves/SIMD]']} waves/SIMD, static LDS {cur['LDS Size [bytes/block]']}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--prompt", type=int, default=3047)
    ap.add_argument("--new_tokens", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3, help="pairs per order (>= 3 in all)")
    ap.add_argument("--launches", action="store_true", help="table (a)")
    ap.add_argument("--loop", action="store_true", help="table (b): builds the full-size decoder")
    ap.add_argument("--resources", action="store_true", help="the compiler report (no GPU needed)")
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

    if a.launches or a.loop:
        import torch
        dev = torch.device("cuda:0")
        log(f"# decode attention, valu vs mfma: {torch.cuda.get_device_name(0)}")
        max_len = -(-(a.prompt + a.new_tokens) // 256) * 256
        if a.launches:
            launches(dev, log, max_len, a.prompt, a.pairs)
            save()
            torch.cuda.empty_cache()
        if a.loop:
            loop(dev, log, save, a.prompt, a.new_tokens, a.pairs)
    if a.resources:
        resources(log)
    save()


if __name__ == "__main__":
    main()
