"""Bit parity of the caption's attention kernels between two builds of the library (the run of tools/gemv_merge_parity.py: two child
processes, one per build, the parent compares with ``torch.equal``): the flash prefill and the decode step of csrc/prefill_attention.hip
and csrc/decode_attention.hip on the exact and adversarial inputs of tests/caption_attention_cases.py.
  * every case of ``all_cases``, fp16 and bf16: the prefill's output; the decode step's output and both caches after it, through the
    single entry (``ops.llama_decode_attention``) on the ``valu`` and the ``mfma`` kernel;
  * the ``_rows`` entry on both kernels at B = 1, 3 and 8: windows over the positions of ``DECODE_POSITIONS`` (one cache length) and of
    ``COMBINE_ROWS`` (8 192 keys and more: da_combine_kernel's second round), outputs and both caches.

    python tools/caption_attention_parity.py --other /path/to/other/librsvld_hip.so [--out profiles/caption_attention_core_parity.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = ("valu", "mfma")
ROWS = (1, 3, 8)


def compute(path):
    import torch
    import caption_attention_cases as CA
    from rsvld_amd import decode_rows as DR, ops, prefill_attention as PA
    dev = torch.device("cuda:0")
    out = {}

    def put(key, *tensors):
        assert key not in out, key
        out[key] = torch.cat([t.flatten() for t in tensors]).cpu()

    for dtype in CA.DTYPES:
        dn = CA.DTN[dtype]
        for c in CA.all_cases(dtype):
            if c.kind == "prefill":
                put(f"prefill flash {dn} {c.label}", PA.llama_prefill_attention(c.q.to(dev), c.k.to(dev), c.v.to(dev), c.n_q, c.n_kv, CA.SCALE, pos0=c.pos0))
                continue
            for kernel in KERNELS:
                kc, vc = c.kc.to(dev), c.vc.to(dev)
                o = ops.llama_decode_attention(c.qkv.to(dev), c.cos.to(dev), c.sin.to(dev), torch.tensor([c.pos], device=dev), kc, vc, c.n_q, c.n_kv,
                                               CA.SCALE, kernel=kernel)
                put(f"decode {kernel} {dn} {c.label}", o, kc, vc)
        # the _rows entry: B sequences of one cache length, the positions taken cyclically from each list
        lists = {"decode": ((8, 2), 384, [p for m, p in CA.DECODE_POSITIONS if m == 384]), "combine": (CA.COMBINE_GROUP, CA.COMBINE_MAX_LEN, CA.COMBINE_ROWS)}
        for name, ((n_q, n_kv), max_len, positions) in lists.items():
            cases = [CA.ramp_decode(n_q, n_kv, max_len, p, dtype, "saw") for p in positions]
            for B in ROWS:
                for first in range(len(cases) if B < 8 else 1):
                    cs = [cases[(first + j) % len(cases)] for j in range(B)]
                    stack = lambda f: torch.stack([getattr(c, f) for c in cs]).to(dev)
                    for kernel in KERNELS:
                        kb, vb = stack("kc"), stack("vc")
                        o = DR.llama_decode_attention_rows(stack("qkv"), stack("cos"), stack("sin"), torch.tensor([c.pos for c in cs], device=dev), kb, vb,
                                                           n_q, n_kv, CA.SCALE, kernel=kernel)
                        put(f"rows {kernel} {dn} {name} B={B} positions {[c.pos for c in cs]}", o, kb, vb)
    torch.cuda.synchronize()
    torch.save(out, path)


if __name__ == "__main__":
    import gemv_merge_parity
    sys.exit(gemv_merge_parity.main(compute=compute, script=os.path.abspath(__file__), what="caption attention kernels", doc=__doc__))
