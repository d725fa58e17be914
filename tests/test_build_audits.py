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


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "remote-sensing-vision-language-diffusion-model_amd", "csrc")
LAUNCH_SITES = 93
# what may stand as the stream of a launch, and why each is the entry point's ``void* stream``:
#   (hipStream_t)stream   the parameter itself, cast
#   s                     a local ``hipStream_t s = (hipStream_t)stream;`` of the entry point, or the ``hipStream_t s`` parameter of a
#                         file-local launch helper, whose every caller passes one of these three spellings in that position
#   l.s                   attention.hip's launch record, filled by its one ``l.s = (hipStream_t)stream;``
STREAM_SPELLINGS = ("(hipStream_t)stream", "s", "l.s")
# every way the type name may appear in the library at all: nothing else can bring a stream into being
STREAM_TYPE_USES = (r"hipStream_t s = \(hipStream_t\)stream;", r"\(hipStream_t\)stream\b", r"hipStream_t s(?=[,)])", r"hipStream_t s;")


def _strip_comments(src):
    import re
    src = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _call_args(src, open_paren):
    """The top-level arguments of the call whose ``(`` is at ``open_paren`` (brackets of every kind nest; the template brackets
    of a kernel name sit inside its own parentheses or hold no comma), and the index past its ``)``."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(src)):
        c = src[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(" ".join(src[start:i].split()))
                return args, i + 1
        elif c == "," and depth == 1:
            args.append(" ".join(src[start:i].split()))
            start = i + 1
    raise AssertionError("unbalanced call")


def _helper_calls(src, name, defined_at):
    """[(arguments, offset)] of every call of the file-local function ``name`` (its definition at ``defined_at`` left out)."""
    import re
    calls = []
    for c in re.finditer(r"\b%s\b\s*" % name, src):
        if c.start() == defined_at:
            continue
        at_paren = c.end()
        if src[at_paren] == "<":       # explicit template arguments (nested: helper<kernel<f16, 1>, SMEM>, helper<decltype(io)>)
            depth = 0
            while True:
                depth += {"<": 1, ">": -1}.get(src[at_paren], 0)
                at_paren += 1
                if depth == 0:
                    break
            at_paren += len(src[at_paren:]) - len(src[at_paren:].lstrip())
        if src[at_paren] != "(":       # "(cond ? helper<f16> : helper<bf16>)(args)": the call follows the enclosing parentheses
            depth = 0
            while depth >= 0:
                depth += {"(": 1, ")": -1}.get(src[at_paren], 0)
                at_paren += 1
            assert src[at_paren] == "(", (name, src[c.start():at_paren + 1])
        calls.append((_call_args(src, at_paren)[0], c.start()))
    return calls


def _sources(pattern=(".hip", ".h", ".inc")):
    return {f: _strip_comments(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith(pattern)}


def test_every_launch_runs_on_the_callers_stream():
    """A launch that drops the stream, or passes 0, goes to the null stream: invisible to every test that runs on the default
    stream, a data race where infer.py issues the VAE passes on a side stream.  Every ``hipLaunchKernelGGL`` of csrc/ passes, as its
    fifth argument, a listed spelling that is the entry point's ``stream`` (``STREAM_SPELLINGS``); the helpers that take a
    ``hipStream_t s`` are given one of the same spellings by each of their callers; the type name appears in no other form; and
    nothing in the library synchronises, copies or fills on a stream of its own choosing."""
    import re
    srcs = _sources()
    sites = []
    for f, src in srcs.items():
        for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", src):
            args, _ = _call_args(src, m.end() - 1)
            sites.append((f, src.count("\n", 0, m.start()) + 1, args))
    assert all(f.endswith(".hip") for f, _, _ in sites), "a launch outside csrc/*.hip"
    assert len(sites) == LAUNCH_SITES, len(sites)
    for f, line, args in sites:
        assert len(args) >= 5, (f, line, args)
        # the kernel name of a two-parameter template is parenthesised, or the macro would split at its comma: then the stream
        # would not be argument five and the next assertion fails
        assert args[4] in STREAM_SPELLINGS, f"{f}:{line}: the launch runs on '{args[4]}'"
        assert args[4] not in ("0", "nullptr", "NULL")
    used = {a[4] for _, _, a in sites}
    assert used == set(STREAM_SPELLINGS), used
    for f, src in srcs.items():
        assert "<<<" not in src, f"{f}: a <<< >>> launch"
        # no other use of the type; no stream of the library's own
        rest = src
        for pat in STREAM_TYPE_USES:
            rest = re.sub(pat, "", rest)
        assert "hipStream" not in rest, f"{f}: {re.search(r'[^;]*hipStream[^;]*', rest).group(0).strip()}"
        if "l.s" in {a[4] for g, _, a in sites if g == f}:
            assert re.findall(r"\bl\.s\s*=[^=][^;]*;", src) == ["l.s = (hipStream_t)stream;"], f
        # the helpers with a stream parameter: each caller hands its own stream on
        helpers = []
        for m in re.finditer(r"\b(\w+)\s*\(([^()]*\bhipStream_t s\b[^()]*)\)\s*\{", src):
            params = [p.split() for p in m.group(2).split(",")]
            at = [i for i, p in enumerate(params) if p[-2:] == ["hipStream_t", "s"]]
            assert len(at) == 1 and not m.group(1).startswith("rsvld_"), (f, m.group(1))
            helpers.append((m.group(1), m.start(), at[0] - len(params), len(params)))
        for name, defined_at, from_end, nparams in helpers:      # grows: a forwarder found below is a helper too
            calls = _helper_calls(src, name, defined_at)
            assert calls, (f, name)
            for args, call_at in calls:
                if args == ["a..."]:
                    # forwarded as a parameter pack (gemv.hip's switch over the row count): the stream must be the helper's last
                    # parameter, and the forwarding function is held to the same rule, whatever stands before the pack
                    assert from_end == -1, (f, name)
                    fw = [m for m in re.finditer(r"\b(\w+)\s*\([^()]*\bA\.\.\. a\)\s*\{", src[:call_at])][-1]
                    if all(h[0] != fw.group(1) for h in helpers):
                        helpers.append((fw.group(1), fw.start(), -1, None))
                    continue
                assert nparams is None or len(args) == nparams, (f, name, args)
                assert args[from_end] in STREAM_SPELLINGS, f"{f}: {name}(...) is given the stream '{args[from_end]}'"
    # host-side calls that pick a stream themselves (the null stream) or stall the caller's
    hits = [(f, m.group(0)) for f, src in srcs.items() for m in re.finditer(r"\bhip\w*Synchronize\w*|\bhipMemset\w*|\bhipMemcpy\w*", src)]
    assert hits == [("gemm.hip", "hipMemcpyFromSymbol")], hits
    gemm = srcs["gemm.hip"]
    i = gemm.index("hipMemcpyFromSymbol")
    assert "rsvld_debug_gemm_stamps" in gemm[gemm.rindex("\n}", 0, i):i]


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
