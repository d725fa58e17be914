"""Audit for the inline-asm LDS-DMA statements that declare M0 clobbered instead of saving / restoring it (attn_d512b_kernel, gemm256_kernel):
hipcc reserves M0 and warns that clobbering it "may lead to undefined behaviour", so the build is only acceptable while the
COMPILER itself never reads or writes M0 in that translation unit.  Compiles the units to assembly and fails if M0 appears
anywhere outside an ;;#ASMSTART .. ;;#ASMEND block.   python tools/audit_m0.py [extra hipcc flags]
(tests/test_build_audits.py runs it for gemm.hip, whose shipped build has such statements.)"""
import os, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_units

# translation units whose inline-asm LDS-DMA statements clobber M0 (flags and compile command: device_units)
UNITS = ["attention.hip", "gemm.hip"]


def audit(unit="attention.hip", extra=()):
    bad, inasm, dma = [], False, 0
    for n, line in enumerate(device_units.assembly(unit, extra=extra).splitlines(), 1):
        if "#ASMSTART" in line:
            inasm = True
        elif "#ASMEND" in line:
            inasm = False
        else:
            code = line.split(";")[0]
            if inasm and "global_load_lds" in code:
                dma += 1
            if not inasm and "m0" in code.replace("vm0", "") and not code.strip().startswith("."):
                bad.append((n, line.strip()))
    return bad, dma


if __name__ == "__main__":
    rc = 0
    for unit in UNITS:
        bad, dma = audit(unit, sys.argv[1:])
        print(f"{unit}: {dma} LDS-DMA instructions inside asm blocks; compiler uses of m0 outside asm blocks: {len(bad)}")
        for n, l in bad[:20]:
            print(f"  line {n}: {l}")
        rc |= 1 if bad else 0
    sys.exit(rc)
