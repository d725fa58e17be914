"""The attention case lists of the GPU tests, walked on the CPU: every claim they make about the route of a shape -- which kernel, how
many key ranges, whether a workspace is needed -- is put to the library's own planner (rsvld_plan_attention: host code, no device), and
together the cases must reach every row of the launch table of csrc/attention.hip on both 16-bit types.  Needs the built library, as
tests/test_cabi.py does."""
import re
from pathlib import Path

import test_gpu_attn_d512_dsplit as DS
import test_gpu_fullkeys as FK
import test_gpu_guarded as GD
import test_gpu_kernels as K
from test_gpu_kernels import attn_plan

CSRC = Path(__file__).resolve().parents[1] / "remote-sensing-vision-language-diffusion-model_amd" / "csrc"
TUNE64 = {"": 0, "b": 1, "c": 2}               # RSVLD_ATTN_D64_*
TUNE512 = {"": 0, "rows": 4, "dsplit": 5}      # RSVLD_ATTN_D512_*


def _d64_forced(form, shape):
    """A forced d = 64 form: ``b`` runs attn_d64b; ``c`` runs attn_d64c wherever there is more than one 64-key tile (its ring is
    primed with the second one), else attn_d64b as well."""
    B, heads, Nq, Nk = shape
    name = attn_plan(B, heads, Nq, Nk, 64, tune=TUNE64[form], k_ts=2 * heads * 64, v_ts=2 * heads * 64).name
    assert name.startswith("d64b") if (form == "b" or Nk <= 64) else name == "d64c", (form, shape, name)
    return name


def test_d512_kernel_cases_split_as_claimed():
    for (B, Nq, Nk), ranges in K.ATTN_D512_SHAPES.items():
        plan = attn_plan(B, 1, Nq, Nk, 512)
        assert (plan.name, plan.nsplit, plan.ws_bytes > 0) == ("d512b", ranges, ranges > 1)
    assert {K.ATTN_D512_SHAPES[s] for s in ((2, 1024, 1024), (1, 300, 2500))} == {4, 9}
    for (B, Nq, Nk) in K.ATTN_D512_SHARED_SHAPES:
        assert attn_plan(B, 1, Nq, Nk, 512, shared=True).name == "d512d"


def test_d512_dsplit_cases_split_as_claimed():
    assert len(DS.RANGES) == len(DS.CASES)
    want = {(1, 4096, 4096): 8, (1, 1000, 262144): 16, (1, 65536, 65536): 1, (1, 24653, 2053): 1}
    for (B, Nq, Nk, plan_div, _), ranges in zip(DS.CASES, DS.RANGES):
        assert want.get((B, Nq, Nk), ranges) == ranges
        for kernel, row in (("", "d512d"), ("dsplit", "d512d"), ("rows", "d512b_shared")):
            plan = attn_plan(B, 1, Nq, Nk, 512, plan_div=plan_div, tune=TUNE512[kernel], shared=True)
            assert (plan.name, plan.nsplit) == (row, ranges)


def test_guarded_cases_route_as_their_names_claim():
    named = 0
    for name, shape, kernel, plan_div, shared in GD.ATTN512:
        plan = GD.attn512_plan(name, shape, kernel, plan_div, shared)      # asserts split_kv / unsplit in the name
        named += "split_kv" in name or "unsplit" in name
        assert plan.name == ("d512b" if not shared else "d512b_shared" if kernel == "rows" else "d512d")
    assert named >= 3
    assert {f for f, _ in GD.ATTN64} == {"b", "c"}
    for form, shape in GD.ATTN64:
        _d64_forced(form, shape)


def test_full_size_cases_route_as_claimed():
    B, heads, Nq, Nk = FK.D64_PINGPONG_SHAPE
    assert attn_plan(B, heads, Nq, Nk, 64, k_ts=3 * heads * 64, v_ts=3 * heads * 64).name == "d64c"
    assert (Nq + 511) // 512 * heads * B == 1024        # the grid its docstring names
    for shared in (False, True):
        plan = attn_plan(1, 1, 262144, 262144, 512, shared=shared)
        assert (plan.nsplit, plan.keys_per_split) == (4, 65536)


def test_the_cases_reach_every_row_of_the_launch_table_on_both_types():
    from rsvld_amd import _lib as L
    src = (CSRC / "attention.hip").read_text()
    table = src[src.index("ATTN_TABLE[6][2]"):]
    table = table[:table.index("};")]
    assert len(re.findall(r"^\s*ATTN_ROW(?:64|512)\(", table, re.M)) == len(L.ATTN_ROW) == 6
    assert not re.search(r"hipLaunchKernelGGL\(\(?attn_", src), "an instantiation is launched outside the table"
    seen = set()                                       # (row, dtype) over the kernel-level tests, each of which runs on DTYPES
    for dtype in K.DTYPES:
        seen |= {(attn_plan(B, 1, Nq, Nk, 512).name, dtype) for B, Nq, Nk in K.ATTN_D512_SHAPES}
        seen |= {(_d64_forced(form, shape), dtype) for shape in K.ATTN_D64_SHAPES for form in "bc"}
        for (B, heads, Nq, Nk), row, other in K.ATTN_D64_DEFAULT_CASES:
            assert attn_plan(B, heads, Nq, Nk, 64, k_ts=2 * heads * 64, v_ts=2 * heads * 64).name == row
            assert _d64_forced(other, (B, heads, Nq, Nk))[:4] != row[:4]       # the forced form is the OTHER kernel
            seen.add((row, dtype))
    for dtype in DS.DTYPES:
        for B, Nq, Nk, plan_div, _ in DS.CASES:
            seen |= {(attn_plan(B, 1, Nq, Nk, 512, plan_div=plan_div, tune=t, shared=True).name, dtype) for t in TUNE512.values()}
    assert seen == {(row, dtype) for row in L.ATTN_ROW for dtype in K.DTYPES}, seen
    assert set(K.DTYPES) == set(DS.DTYPES) and len(K.DTYPES) == 2


def test_dynamic_lds_sizes_are_registered_in_one_place():
    """rsvld_smem_once (csrc/rsvld_common.h), keyed on the kernel, is the library's only hipFuncSetAttribute."""
    calls = {p.name: len(re.findall(r"hipFuncSetAttribute\(", p.read_text())) for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".inc", ".h")}
    assert {n: c for n, c in calls.items() if c} == {"rsvld_common.h": 1}
