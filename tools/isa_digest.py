"""Per-kernel digests of the device assembly of every unit of csrc/Makefile (the table and the compile command of tools/device_units.py),
to show that a source change left the shipped instruction streams alone.  A kernel's text runs from its label to
.end_amdhsa_kernel, without ';' comments, trailing blanks and the function index in local labels (.LBB10_65 -> .LBB_65, likewise
.Lfunc_end / .Ltmp); the digest is the first 16 hex digits of its sha256.
    python tools/isa_digest.py [--mask] [--resources] [--pair OLD=NEW ...] [csrc directory of another checkout, e.g. the parent commit's] [unit ...]
An argument that names a unit (attention.hip, split.hip, ...) restricts the table to the units named; without one, all.
One line per kernel: unit, symbol, [the other checkout's digest and instruction-line count,] this tree's digest and count
('-' where a tree has no such kernel).  profiles/attn_prune_isa.txt and profiles/gemm_prune_isa.txt are such tables.

--mask compares kernels across a rename (template arguments are part of a symbol): the kernel's own mangled symbol is replaced by
@KERNEL inside its text before hashing, and a kernel of the other checkout that this tree no longer has is put on one line with its
successor, whose symbol is appended as "-> symbol".  The successor comes from --pair OLD=NEW (mangled symbols) or from RENAMES below;
profiles/norm_merge_isa.txt is such a table.  Without --mask nothing is masked or paired.

A kernel that moved to another unit keeps its symbol: MOVED names, per unit of this tree, the units of the other checkout its kernels
came from, and the table of that unit sets them beside the other checkout's kernels of the same symbol (the unit they left shows them
with '-' for this tree).  profiles/caption_attention_core_isa.txt is such a table.

--resources appends, per digest, next_free_vgpr:NumVgprs:NumAgprs:LDS-bytes:scratch-instructions (the kernel descriptor's
next_free_vgpr is what the launch bounds let the compiler allot; NumVgprs / NumAgprs are what the code uses)."""
import hashlib, os, re, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_units

HERE = device_units.CSRC
UNITS = list(device_units.UNITS)
# units of another checkout whose kernels live in this unit today (built there with this unit's flags)
MOVED = {"decode_attention.hip": ["gemv.hip", "decode_attention_mma.hip"]}
# renamed kernels, per unit: (regex over the start of the old symbol, the start of its successor's symbol as a template of the match)
N = "_ZN12_GLOBAL__N_1"
RENAMES = {"norm.hip": [
    (N + r"17gn_partial_kernelI(DF16_|DF16b)E", N + r"17gn_partial_kernelINS_4Io16I\1EEE"),
    (N + r"21gn_partial_f32_kernelE", N + r"17gn_partial_kernelINS_5IoF32ILi1EEEE"),
]}


def digests(src, unit, mask=False, resources=False, flags=None):
    text = device_units.assembly(unit, src, flags)
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
        if resources:
            tail = text[text.index(".amdhsa_kernel " + k):]
            desc = dict(re.findall(r"^\s*\.amdhsa_(\w+)\s+(\d+)", tail[:tail.index(".end_amdhsa_kernel")], re.M))
            used = dict(re.findall(r"^; (NumVgprs|NumAgprs): (\d+)", text[text.index(k + ":"):], re.M)[:2])
            rows[k] += (f"{desc['next_free_vgpr']}:{used['NumVgprs']}:{used['NumAgprs']}:{desc['group_segment_fixed_size']}:{body.count('scratch_')}",)
    return rows


def other_digests(other, unit, have, **kw):
    """the other checkout's kernels of `unit`, and of the units that `unit`'s kernels (`have`) came from"""
    old = digests(other, unit, **kw) if os.path.exists(os.path.join(other, unit)) else {}
    for src in MOVED.get(unit, []):
        if os.path.exists(os.path.join(other, src)):
            old.update({k: v for k, v in digests(other, src, flags=device_units.UNITS[unit], **kw).items() if k in have or src not in UNITS})
    return old


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
    mask, resources = "--mask" in args, "--resources" in args
    pairs = dict(args[i + 1].split("=", 1) for i, a in enumerate(args[:-1]) if a == "--pair")
    args = [a for i, a in enumerate(args) if a not in ("--mask", "--resources", "--pair") and (i == 0 or args[i - 1] != "--pair")]
    units = [a for a in args if a in UNITS]
    dirs = [a for a in args if a not in UNITS]
    if len(dirs) > 1 or (dirs and not os.path.isdir(dirs[0])):
        sys.exit(f"isa_digest.py: expected at most one csrc directory and units out of {', '.join(UNITS)}: {' '.join(dirs)}")
    other = os.path.abspath(dirs[0]) if dirs else None
    print("# " + subprocess.run([device_units.HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    cols = "digest lines" + (" next_free_vgpr:vgprs:agprs:lds:scratch" if resources else "")
    print("# unit symbol " + (" ".join("other-" + c for c in cols.split()) + " " if other else "") + cols + (" [-> successor symbol]" if mask and other else ""))
    for unit in units or UNITS:
        new = digests(HERE, unit, mask, resources)
        old = other_digests(other, unit, new, mask=mask, resources=resources) if other else {}
        blank = ("-",) * (3 if resources else 2)
        fresh = [k for k in new if k not in old]
        for k in list(old):
            succ = successor(unit, k, fresh, pairs) if mask and k not in new else None
            if succ:
                fresh.remove(succ)
            print(unit, k, *old[k], *new.get(succ or k, blank), *(("->", succ) if succ else ()))
        for k in fresh:
            print(unit, k, *(blank if other else ()), *new[k])
