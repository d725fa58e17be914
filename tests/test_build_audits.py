"""Build-time audits of the hand-scheduled kernels (CPU: hipcc cross-compiles gfx950 assembly here)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


import pytest


@pytest.mark.parametrize("unit", ["gemm.hip", "attention.hip"])
def test_compiler_never_touches_m0_beside_the_asm_lds_dma(unit):
    """The LDS-DMA pieces of gemm256_kernel and attn_d512b_kernel are inline asm that writes M0 (the LDS destination) and declares
    it clobbered instead of saving / restoring it; hipcc reserves M0 and only warns.  The build is sound as long as the compiler
    itself never reads or writes M0 in that translation unit: every M0 use in the assembly must sit inside an
    ;;#ASMSTART .. ;;#ASMEND block."""
    import audit_m0
    bad, dma = audit_m0.audit(unit)
    assert dma >= 16, dma            # the pieces are really there
    assert not bad, bad[:5]


@pytest.mark.parametrize("unit", ["conv_igemm.hip", "conv_halo.hip", "gemm.hip", "split.hip"])
def test_lds_dma_kernels_use_no_scratch(unit):
    """A spill or a compiler-built stack table inside a kernel that streams its operands by LDS-DMA is reloaded with scratch_load,
    which shares vmcnt with the DMA ring: the wait in front of the reload drains the prefetch (round 4: conv_igemm 586 -> 437 TFLOP/s
    from a runtime flag in its source selection).  No MFMA kernel of these units may contain a scratch instruction."""
    import audit_scratch
    res = audit_scratch.audit(unit)
    assert len(res) >= 3 or unit == "split.hip", res   # the MFMA kernels are really there
    if unit == "split.hip":   # its two: the split attention kernels
        assert len(res) == 2 and any("attn_split_d64_kernel" in k for k in res) and any("attn_split_d512_kernel" in k for k in res), res
    bad = {k: v for k, v in res.items() if v > 0}
    assert not bad, bad


def test_the_device_unit_table_is_the_makefiles():
    """tools/device_units.py (the compile command of isa_digest.py, audit_scratch.py and audit_m0.py) names every unit of csrc/Makefile's
    SRCS, in its order, with the flags of the unit's EXTRA line -- and nothing else -- so the audits read the code the library ships."""
    import re
    import device_units
    mk = open(os.path.join(device_units.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    extra = {m.group(1) + ".hip": m.group(2).split() for m in re.finditer(r"^\$\(ROOT\)/build/(\w+)\.o: EXTRA := (.*)$", mk, re.M)}
    assert len(srcs) >= 15 and extra, (srcs, extra)             # the two patterns still match the Makefile
    assert set(extra) <= set(srcs), extra
    assert list(device_units.UNITS) == srcs
    assert {u: list(f) for u, f in device_units.UNITS.items()} == {u: extra.get(u, []) for u in srcs}
    import audit_m0, audit_scratch, isa_digest
    assert set(audit_m0.UNITS) | set(audit_scratch.UNITS) <= set(srcs) and list(isa_digest.UNITS) == srcs
