"""Bit parity of the decode operators between two builds of the library: every entry point of csrc/gemv.hip on the shapes of
tests/test_gpu_decode_rows.py (the smallest that reach each loop of the kernel), plus one K near the single-row LDS limit, and the token
loops of a seeded small Llama.  Two child processes compute the same outputs, one on the build RSVLD_LIB-style given by --other (e.g. the
parent commit's librsvld_hip.so), one on this tree's build; the parent process compares them with ``torch.equal`` and prints one line per
group of cases.  The single-row functions reach each build's single-row entry points, the ``_rows`` functions its multi-row ones.

    python tools/gemv_merge_parity.py --other /path/to/other/librsvld_hip.so [--out profiles/gemv_merge_parity.txt]

tools/caption_attention_parity.py is the same run (``main`` below) over the caption's attention kernels.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NATIVE_SHAPES = [(37, 1544), (20, 2048), (20, 4096), (24, 14336), (8, 32640)]     # (8, 32 640): groups of two rows (8 -> 4 x 2)
W8_SHAPES = [(17, 16), (37, 1552), (20, 3584), (24, 14336), (8, 32640)]
PROMPTS, NEW, MAX_LEN = (5, 131, 300), 24, 512


def compute(path):
    import torch
    from rsvld_amd import decode_rows as DR, llava_next as LN, ops, w8
    dev = torch.device("cuda:0")
    out = {}
    for dtype, dn in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for kind, shapes in (("native", NATIVE_SHAPES), ("e4m3", W8_SHAPES)):
            for N, K in shapes:
                g = torch.Generator().manual_seed(1000 * N + K)
                w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, dtype)
                x = torch.randn(8, K, generator=g).to(dev, dtype)
                gu = torch.randn(8, 2 * K, generator=g).to(dev, dtype)
                res = torch.randn(8, N, generator=g).to(dev, dtype)
                b = (torch.randn(N, generator=g) * 0.1).to(dev, dtype)
                nw = (torch.randn(K, generator=g) * 0.2 + 1).to(dev, dtype)
                if kind == "e4m3":
                    q, scale = w8.pack_rows_e4m3(w)
                    out[f"gemv {kind} {dn} {N}x{K} pack"] = torch.cat([q.flatten().float(), scale]).cpu()
                    single = lambda a, bias, **kw: w8.gemv_w8(q, scale, a, bias, **kw)
                    rows = lambda a, bias, **kw: DR.gemv_w8_rows(q, scale, a, bias, **kw)
                else:
                    single = lambda a, bias, **kw: ops.gemv_fused(w, a, bias, **kw)
                    rows = lambda a, bias, **kw: DR.gemv_rows(w, a, bias, **kw)
                    out[f"gemv {kind} {dn} {N}x{K} ops.gemv"] = torch.stack([ops.gemv(w, x[r], b) for r in range(8)]).cpu()
                forms = {"plain": (x, None, {}), "norm": (x, None, {"norm": (nw, 1e-5)}), "glu_residual": (gu, None, {"glu": True, "residual": res}),
                         "bias_residual": (x, b, {"residual": res})}
                for name, (act, bias, kw) in forms.items():
                    row_kw = lambda r: {k: (v[r] if k == "residual" else v) for k, v in kw.items()}
                    out[f"gemv {kind} {dn} {N}x{K} {name} single"] = torch.stack([single(act[r], bias, **row_kw(r)) for r in range(8)]).cpu()
                    for B in range(1, 9):
                        kb = {k: (v[:B].contiguous() if k == "residual" else v) for k, v in kw.items()}
                        out[f"gemv {kind} {dn} {N}x{K} {name} B={B}"] = rows(act[:B].contiguous(), bias, **kb).cpu()
        n_q, n_kv, hd, max_len = 8, 2, 128, 384
        for positions in ((0, 128, 300), (383, 5, 200)):
            B = len(positions)
            g = torch.Generator().manual_seed(7)
            qkv = torch.randn(B, (n_q + 2 * n_kv) * hd, generator=g).to(dev, dtype)
            ang = torch.rand(B, hd, generator=g) * 6.28
            cos, sin = torch.cos(ang).to(dev, dtype), torch.sin(ang).to(dev, dtype)
            kc = torch.randn(B, n_kv, max_len, hd, generator=g).to(dev, dtype)
            vc = torch.randn(B, n_kv, max_len, hd, generator=g).to(dev, dtype)
            pos = torch.tensor(positions, device=dev)
            tag = f"attention {dn} pos={positions}"
            for s in range(B):
                k1, v1 = kc[s].clone(), vc[s].clone()
                o = ops.llama_decode_attention(qkv[s], cos[s], sin[s], pos[s:s + 1].clone(), k1, v1, n_q, n_kv, hd ** -0.5)
                out[f"{tag} single seq {s}"] = torch.cat([o.flatten(), k1.flatten(), v1.flatten()]).cpu()
            kb, vb = kc.clone(), vc.clone()
            o = DR.llama_decode_attention_rows(qkv, cos, sin, pos, kb, vb, n_q, n_kv, hd ** -0.5)
            out[f"{tag} rows"] = torch.cat([o.flatten(), kb.flatten(), vb.flatten()]).cpu()
    # the seeded Llama of tests/test_gpu_decode_rows.py: greedy and seeded-sampled tokens through generate and generate_batch
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=2000, hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, max_position_embeddings=1024, rms_norm_eps=1e-5, rope_theta=500000.0, attention_bias=False)
    torch.manual_seed(11)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(2.0)
        model.to(device=dev, dtype=torch.float16)
        embs = [model.model.embed_tokens(torch.randint(0, cfg.vocab_size, (1, n), generator=torch.Generator().manual_seed(20 + n)).to(dev))
                for n in PROMPTS]
        seeds = [1, 2, 3]
        for weights in LN.FastDecoder.WEIGHTS:
            dec = LN.FastDecoder(model, MAX_LEN, weights=weights, batch=3)
            for i, e in enumerate(embs):
                out[f"tokens {weights} generate greedy prompt {i}"] = dec.generate(e, NEW, do_sample=False).cpu()
                with torch.random.fork_rng(devices=[dev]):
                    torch.manual_seed(seeds[i])
                    out[f"tokens {weights} generate sampled prompt {i}"] = dec.generate(e, NEW, do_sample=True, temperature=0.7).cpu()
            for i, t in enumerate(dec.generate_batch(embs, NEW, do_sample=False)):
                out[f"tokens {weights} generate_batch greedy prompt {i}"] = t.cpu()
            for i, t in enumerate(dec.generate_batch(embs, NEW, do_sample=True, temperature=0.7, seeds=seeds)):
                out[f"tokens {weights} generate_batch sampled prompt {i}"] = t.cpu()
    torch.cuda.synchronize()
    torch.save(out, path)


def main(argv=None, compute=compute, script=os.path.abspath(__file__), what="decode operators", doc=__doc__):
    """``compute(path)`` saves {case: CPU tensor} in a child process per build (``script --child path``); the cases are grouped by their
    first three words (four for a product)."""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--other", help="the other build of librsvld_hip.so")
    ap.add_argument("--out", default=None, help="also write the summary to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return compute(a.child)
    if not a.other or not os.path.exists(a.other):
        sys.exit(f"{os.path.basename(script)}: --other must name the other build of the library")
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for name, lib in (("other", os.path.abspath(a.other)), ("tree", None)):
            env = dict(os.environ)
            env.pop("RSVLD_LIB", None)
            if lib:
                env["RSVLD_LIB"] = lib
            path = os.path.join(tmp, name + ".pt")
            subprocess.run([sys.executable, script, "--child", path], env=env, check=True, timeout=600)
            got[name] = torch.load(path)
    lines = [f"# {what}, the other build against this tree's, torch.equal per case ({torch.__version__}); "
             f"single-row functions on each build's single-row entry points"]
    groups, bad = {}, []
    assert got["other"].keys() == got["tree"].keys()
    for k, v in got["tree"].items():
        o = got["other"][k]
        same = v.shape == o.shape and v.dtype == o.dtype and torch.equal(v.view(torch.uint8) if v.dtype != torch.int64 else v,
                                                                         o.view(torch.uint8) if o.dtype != torch.int64 else o)
        finite = bool(torch.isfinite(v.float()).all())
        grp = " ".join(k.split(" ")[:4]) if k.startswith("gemv") else " ".join(k.split(" ")[:3])
        n, ok = groups.get(grp, (0, 0))
        groups[grp] = (n + 1, ok + int(same and finite))
        if not (same and finite):
            bad.append(k)
    for grp, (n, ok) in groups.items():
        lines.append(f"{grp}: {ok} of {n} cases equal and finite")
    lines.append(f"total: {sum(ok for _, ok in groups.values())} of {len(got['tree'])} cases equal; differing: {bad if bad else 'none'}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
