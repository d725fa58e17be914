"""The translation units of csrc/Makefile with their per-unit flags (its EXTRA lines), and the one command that compiles a unit to gfx950
device assembly with the Makefile's flags.  tools/isa_digest.py, tools/audit_scratch.py and tools/audit_m0.py compile through it;
tests/test_build_audits.py holds the table against the Makefile."""
import os, subprocess, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SLP = ["-fno-slp-vectorize"]
UNITS = {"conv_igemm.hip": [], "conv_halo.hip": [], "gemm.hip": [], "norm.hip": [], "attention.hip": SLP, "elementwise.hip": [],
         "sampler.hip": [], "f32.hip": [], "gemv.hip": [], "split.hip": SLP, "image.hip": [], "prefill_attention.hip": SLP, "gemm_w8.hip": [],
         "gemv_mma.hip": [], "decode_attention.hip": []}


def assembly(unit, csrc=CSRC, flags=None, extra=()):
    """the device assembly of `unit` of the checkout whose csrc directory is given; flags: the unit's own unless given (a unit of another
    checkout that this tree no longer has)"""
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", *(UNITS[unit] if flags is None else flags),
                        f"-I{csrc}", f"-I{inc}", "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, unit), *extra],
                       check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()
