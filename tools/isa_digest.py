"""Per-kernel digests of the device assembly of attention.hip, split.hip and gemm.hip (the compile command of tools/audit_m0.py), to
show that a source change left the shipped instruction streams alone.  A kernel's text runs from its label to .end_amdhsa_kernel,
without ';' comments, trailing blanks and the function index in local labels (.LBB10_65 -> .LBB_65, likewise .Lfunc_end / .Ltmp);
the digest is the first 16 hex digits of its sha256.
    python tools/isa_digest.py [csrc directory of another checkout, e.g. the parent commit's] [unit ...]
An argument that names a unit (attention.hip, split.hip, gemm.hip) restricts the table to the units named; without one, all.
One line per kernel: unit, symbol, [the other checkout's digest and instruction-line count,] this tree's digest and count
('-' where a tree has no such kernel).  profiles/attn_prune_isa.txt and profiles/gemm_prune_isa.txt are such tables."""
import hashlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = {"attention.hip": ["-fno-slp-vectorize"], "split.hip": ["-fno-slp-vectorize"], "gemm.hip": []}   # the Makefile's per-unit flags


def digests(src, unit):
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
        lines = [re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1", l.split(";")[0]).rstrip() for l in body.split("\n")]
        lines = [l for l in lines if l]
        insns = sum(1 for l in lines if l[0] in " \t" and not l.lstrip().startswith("."))
        rows[k] = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], str(insns))
    return rows


if __name__ == "__main__":
    units = [a for a in sys.argv[1:] if a in UNITS]
    dirs = [a for a in sys.argv[1:] if a not in UNITS]
    if len(dirs) > 1 or (dirs and not os.path.isdir(dirs[0])):
        sys.exit(f"isa_digest.py: expected at most one csrc directory and units out of {', '.join(UNITS)}: {' '.join(dirs)}")
    other = os.path.abspath(dirs[0]) if dirs else None
    print("# " + subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    print("# unit symbol " + ("other-digest other-lines " if other else "") + "digest lines")
    for unit in units or UNITS:
        new, old = digests(HERE, unit), digests(other, unit) if other else {}
        for k in list(old) + [k for k in new if k not in old]:
            print(unit, k, *(old.get(k, ("-", "-")) if other else ()), *new.get(k, ("-", "-")))
