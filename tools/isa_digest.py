"""Per-kernel digests of the device assembly of attention.hip, split.hip, gemm.hip, norm.hip, f32.hip, conv_igemm.hip, conv_halo.hip, gemv.hip and prefill_attention.hip (the compile command of
tools/audit_m0.py), to show that a source change left the shipped instruction streams alone.  A kernel's text runs from its label to
.end_amdhsa_kernel, without ';' comments, trailing blanks and the function index in local labels (.LBB10_65 -> .LBB_65, likewise
.Lfunc_end / .Ltmp); the digest is the first 16 hex digits of its sha256.
    python tools/isa_digest.py [--mask] [--pair OLD=NEW ...] [csrc directory of another checkout, e.g. the parent commit's] [unit ...]
An argument that names a unit (attention.hip, split.hip, ...) restricts the table to the units named; without one, all.
One line per kernel: unit, symbol, [the other checkout's digest and instruction-line count,] this tree's digest and count
('-' where a tree has no such kernel).  profiles/attn_prune_isa.txt and profiles/gemm_prune_isa.txt are such tables.

--mask compares kernels across a rename (template arguments are part of a symbol): the kernel's own mangled symbol is replaced by
@KERNEL inside its text before hashing, and a kernel of the other checkout that this tree no longer has is put on one line with its
successor, whose symbol is appended as "-> symbol".  The successor comes from --pair OLD=NEW (mangled symbols) or from RENAMES below;
profiles/norm_merge_isa.txt is such a table.  Without --mask nothing is masked or paired."""
import hashlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = {"attention.hip": ["-fno-slp-vectorize"], "split.hip": ["-fno-slp-vectorize"], "gemm.hip": [],   # the Makefile's per-unit flags
         "norm.hip": [], "f32.hip": [], "conv_igemm.hip": [], "conv_halo.hip": [], "gemv.hip": [],
         "prefill_attention.hip": ["-fno-slp-vectorize"]}
# renamed kernels, per unit: (regex over the start of the old symbol, the start of its successor's symbol as a template of the match)
N = "_ZN12_GLOBAL__N_1"
RENAMES = {"norm.hip": [
    (N + r"17gn_partial_kernelI(DF16_|DF16b)E", N + r"17gn_partial_kernelINS_4Io16I\1EEE"),
    (N + r"21gn_partial_f32_kernelE", N + r"17gn_partial_kernelINS_5IoF32ILi1EEEE"),
]}


def digests(src, unit, mask=False):
    inc = os.path.join(os.path.dirname(os.path.dirname(src)), "include")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", *UNITS[unit],
                        f"-I{src}", f"-I{inc}", "-S", "--cuda-device-only", "-o", out, os.path.join(src, unit)],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    rows = {}
    for k in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = text[re.search(rf"^{re.escape(k)}:", text, re.M).start():]
        body = body[:body.index(".end_amdhsa_kernel")]
        if mask:
            body = body.replace(k, "@KERNEL")
        lines = [re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1", l.split(";")[0]).rstrip() for l in body.split("\n")]
        lines = [l for l in lines if l]
        insns = sum(1 for l in lines if l[0] in " \t" and not l.lstrip().startswith("."))
        rows[k] = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], str(insns))
    return rows


def successor(unit, k, fresh, pairs):
    """the symbol among `fresh` (this tree's kernels that the other checkout lacks) that replaces the other checkout's kernel k"""
    if k in pairs:
        return pairs[k] if pairs[k] in fresh else None
    for pat, repl in RENAMES.get(unit, []):
        m = re.match(pat, k)
        if m:
            hits = [n for n in fresh if n.startswith(m.expand(repl))]
            return hits[0] if len(hits) == 1 else None
    return None


if __name__ == "__main__":
    args = sys.argv[1:]
    mask = "--mask" in args
    pairs = dict(args[i + 1].split("=", 1) for i, a in enumerate(args[:-1]) if a == "--pair")
    args = [a for i, a in enumerate(args) if a not in ("--mask", "--pair") and (i == 0 or args[i - 1] != "--pair")]
    units = [a for a in args if a in UNITS]
    dirs = [a for a in args if a not in UNITS]
    if len(dirs) > 1 or (dirs and not os.path.isdir(dirs[0])):
        sys.exit(f"isa_digest.py: expected at most one csrc directory and units out of {', '.join(UNITS)}: {' '.join(dirs)}")
    other = os.path.abspath(dirs[0]) if dirs else None
    print("# " + subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    print("# unit symbol " + ("other-digest other-lines " if other else "") + "digest lines" + (" [-> successor symbol]" if mask and other else ""))
    for unit in units or UNITS:
        new, old = digests(HERE, unit, mask), digests(other, unit, mask) if other else {}
        fresh = [k for k in new if k not in old]
        for k in list(old):
            succ = successor(unit, k, fresh, pairs) if mask and k not in new else None
            if succ:
                fresh.remove(succ)
            print(unit, k, *old[k], *new.get(succ or k, ("-", "-")), *(("->", succ) if succ else ()))
        for k in fresh:
            print(unit, k, *(("-", "-") if other else ()), *new[k])
