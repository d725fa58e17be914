"""The cases of tests/test_gpu_attention_exact.py, walked on the CPU (tests/attention_cases.py): the builders' premises are PROVEN
here, none is assumed; the library's planner (host code; needs the built library, as tests/test_cabi.py does) routes the 16-bit
shapes as the tables claim; the fp64 evaluator rounded once to a route's output format passes every assertion on every case (the
cases are fair); and every fault of ``FAULTS`` built into that evaluator is rejected on every route it can occur on, in every output
format of the route (the assertions have teeth)."""
import pytest
import torch

import attention_cases as AC
from test_gpu_kernels import attn_plan

ROUTES = sorted(AC.ROUTES)
D512_ROUTES = {"d512b": (0, False), "d512d": (0, True), "d512b_shared": (4, True)}        # route -> (tune, shared) of the planner
# fault -> the routes it can occur on: 6 needs two heads, 7 two batches, 8 a split-KV plan, 10 the GEMM form's pad columns
APPLIES = {f: ROUTES for f in (1, 2, 3, 4, 5, 9)}
APPLIES[6] = ["d64", "f32", "f32_split", "split_d64"]
APPLIES[7] = ["d64", "d512b", "d512d", "d512b_shared", "f32", "f32_split", "split_d64", "split_d512"]
APPLIES[8] = sorted(D512_ROUTES)
APPLIES[10] = ["gemm"]


def _kps(route, shape):
    """Keys per range of the route's split-KV plan (0: one range)."""
    if route not in D512_ROUTES:
        return 0
    B, heads, Nq, Nk, D = shape
    tune, shared = D512_ROUTES[route]
    plan = attn_plan(B, heads, Nq, Nk, D, tune=tune, shared=shared)
    return plan.keys_per_split if plan.nsplit > 1 else 0


def _all_cases():
    seen = {}
    for route in ROUTES:
        for c in AC.route_cases(route):
            seen[id(c)] = c
    return list(seen.values())


def test_the_tables_name_the_shapes_the_kernels_branch_on():
    tiles = sorted({(Nk + 63) // 64 for _, _, _, Nk in AC.D64_SHAPES})
    assert set(tiles) >= {1, 2, 3, 4, 5}                            # attn_d64c requests three tiles in its prologue and rings four
    assert {Nk % 64 == 0 for _, _, _, Nk in AC.D64_SHAPES} == {True, False}                # full and ragged last tiles
    nq = [Nq for _, _, Nq, _ in AC.D64_SHAPES]
    assert min(nq) < 128 < max(nq) and any(n < 512 for n in nq) and any(n > 512 for n in nq)
    # attn_split_d64_kernel's loop switch (t + 2) * 64 <= Nk: steady iterations 0 at <= 127 keys, 1 from 128, 2 from 192
    nks = {s[3] for s in AC.ROUTES["split_d64"]["shapes"]}
    assert {128, 129, 191, 192} <= nks and {max(0, Nk // 64 - 1) for Nk in nks} >= {0, 1, 2}
    assert {(-Nk) % 8 for Nk in AC.GEMM_NK} == {0, 1, 3, 4, 7} and sum(Nk > 2048 for Nk in AC.GEMM_NK) == 2 and AC.GEMM_NQ > 256
    assert {(D, heads) for _, heads, _, _, D, _ in AC.F32_SHAPES} == {(64, 2), (128, 1), (512, 1)}
    assert sum(s[0] == 2 for s in AC.F32_SHAPES) == 1 and sum(s[5] for s in AC.F32_SHAPES) == 1
    for B, heads, Nq, Nk, D, fused in AC.F32_SHAPES:
        assert not fused or Nq == Nk
    for route in ROUTES:                                              # fault 7 / 6 can be shown on the routes APPLIES names
        assert (route in APPLIES[7]) == any(s[0] == 2 for s in AC.ROUTES[route]["shapes"]), route
        assert (route in APPLIES[6]) == any(s[1] >= 2 for s in AC.ROUTES[route]["shapes"] if route != "d64_nw8"), route


def test_every_operand_is_exact_in_both_16_bit_types():
    for c in _all_cases():
        assert AC.representable(c), c.label


def test_needle_leak_distinct_rows_and_targets():
    worst = 0.0
    for c in _all_cases():
        if c.family != "needle":
            continue
        leak = AC.needle_leak(c)
        assert float(leak.max()) < AC.LEAK_BOUND, (c.label, float(leak.max()))
        worst = max(worst, float(leak.max()))
        assert int(c.targets.min()) >= 0 and int(c.targets.max()) < c.Nk
        assert AC.distinct_rows(c.v64) and AC.distinct_rows(c.k64), c.label         # a wrong key is another V row
        assert torch.equal(c.v64, c.v64.round()) and 1 <= float(c.v64.abs().min()) and float(c.v64.abs().max()) <= 8      # ... off by 1 or more
        assert torch.equal(c.q64, AC.NEEDLE_A[c.D] * torch.gather(c.k64, 2, c.targets[..., None].expand_as(c.q64)))
        if c.Nq >= 8:                                                 # every slot of the cycle occurs
            assert {(b + h + r) % 8 for b in range(c.B) for h in range(c.heads) for r in range(c.Nq)} == set(range(8))
    print(f"needle: worst leak 2^{torch.log2(torch.tensor(worst)).item():.1f} (bound 2^-26)")
    c = AC.needle((1, 2, 600, 273, 64))
    last = 64 * (272 // 64)
    assert [AC.needle_target(0, 0, r, 273, 64) for r in range(6)] == [0, 272, last, last - 1, 63, 64]
    assert int(c.targets[0, 1, 0]) == 272 and int(c.targets[0, 0, 5]) == 64


@pytest.mark.parametrize("route,tile", [("d64", 64), ("d512b", 32), ("f32", 32), ("split_d512", 32), ("gemm", 32)])
def test_every_in_tile_offset_is_a_target(route, tile):
    """Over the shapes of a route the needle's targets reach every offset of a key tile."""
    seen = set()
    for c in AC.route_cases(route):
        if c.family == "needle" and c.tile == tile:
            t = c.targets.flatten()
            seen |= set((t % tile).tolist())
    assert seen == set(range(tile)), sorted(set(range(tile)) - seen)


def test_ramp_scores_are_exact_and_span_the_range():
    for c in _all_cases():
        if c.family != "ramp":
            continue
        assert AC.ramp_scores_exact(c), c.label
        assert int(c.nj.min()) >= 0 and int(c.nj.max()) == c.D or (c.profile == "saw" and 1 < c.Nk < c.tile), c.label
        if c.Nk >= c.tile:
            assert int(c.nj.min()) == 0, c.label
            span = float(AC._scores(c.q64, c.k64, c.scale).abs().max())
            assert span == {64: 32.0, 128: 4 * 128 ** 0.5, 512: 2 * 512 ** 0.5}[c.D], (c.label, span)
        if c.Nq >= 4:
            assert set(c.a[0].tolist()) == set(AC.RAMP_A[c.D])       # every head sees +-a, the single head of d = 512 too
        if c.profile == "saw" and c.Nk >= 2 * c.tile:                   # every full tile spans 0 .. D
            assert int(c.nj[c.tile]) == 0 and int(c.nj[2 * c.tile - 1]) == c.D


def test_counting_cases_count():
    for c in _all_cases():
        if c.family != "counting":
            continue
        assert float(c.q64.abs().max()) == 0.0
        assert bool((c.counts.sum(-1) == c.Nk).all()) and bool(((c.v64 == 1).sum(-1) == 1).all()) and bool(((c.v64 != 0).sum(-1) == 1).all())
        assert float(c.counts.max()) < 128                              # round(got Nk) == c_d holds after one bf16 rounding (c_d 2^-9 < 1 / 2)
        if c.heads >= 2 and c.Nk >= 2:
            assert not torch.equal(c.counts[:, 0], c.counts[:, 1]) or c.Nk % c.D == 0, c.label
        if c.B >= 2:
            assert not torch.equal(c.k64[0], c.k64[1]) and not torch.equal(c.v64[0], c.v64[1])


def test_the_planner_routes_the_16_bit_shapes_as_claimed():
    for (B, heads, Nq, Nk) in AC.D64_SHAPES:
        for ts in (1, 2):                                             # k | v separate, and column slices of one fused tensor
            plan = lambda tune: attn_plan(B, heads, Nq, Nk, 64, tune=tune, k_ts=ts * heads * 64, v_ts=ts * heads * 64).name
            assert plan(1) == "d64b_nw4"
            assert plan(2) == ("d64c" if Nk > 64 else "d64b_nw4"), (B, heads, Nq, Nk)
    B, heads, Nq, Nk = AC.D64_NW8_SHAPE
    assert attn_plan(B, heads, Nq, Nk, 64, k_ts=2 * heads * 64, v_ts=2 * heads * 64).name == "d64b_nw8"
    for route, (tune, shared) in D512_ROUTES.items():
        for (B, Nq, Nk), nsplit in AC.D512_SHAPES.items():
            plan = attn_plan(B, 1, Nq, Nk, 512, tune=tune, shared=shared)
            assert (plan.name, plan.nsplit) == (route, nsplit), (route, B, Nq, Nk)
    assert attn_plan(1, 1, 64, 600, 512).keys_per_split == 320           # two ranges of 320 and 280 keys
    assert (2500 + 287) // 288 == 9 and 2500 % 288 and attn_plan(1, 1, 300, 2500, 512).keys_per_split == 288      # the last one ragged
    assert sorted(AC.D512_SHAPES.values())[-3:] == [2, 4, 9]


@pytest.mark.parametrize("route", sorted(D512_ROUTES))
def test_the_needles_targets_lie_in_every_key_range(route):
    """... and, in every range, a row's target lies in another range than its loudest decoy (the non-target key of the highest score)."""
    for shape in AC.ROUTES[route]["shapes"]:
        kps = _kps(route, shape)
        if not kps:
            continue
        c = AC.needle(shape, AC.ROUTES[route]["shared"])
        n = (c.Nk + kps - 1) // kps
        s = AC._scores(c.q64, c.k64, c.scale)
        s.scatter_(-1, c.targets[..., None], float("-inf"))
        decoy = s.argmax(-1) // kps
        tr = c.targets // kps
        assert set(tr.flatten().tolist()) == set(range(n)), shape
        assert set(tr[tr != decoy].flatten().tolist()) == set(range(n)), shape


@pytest.mark.parametrize("route", ROUTES)
def test_the_rounded_fp64_evaluator_passes_every_case(route):
    for fmt in AC.route_fmts(route):
        worst = {}
        for c in AC.route_cases(route):
            r, equal = AC.check(c, AC.round_to(AC.reference(c), fmt), fmt, AC.route_tol(route, fmt))
            assert equal is None or equal, c.label
            worst[c.family] = max(worst.get(c.family, 0.0), r)
        print(f"ideal kernel, {route} [{fmt}]: worst ratio to the bound {worst}")
        assert worst["needle"] == 0.0 and worst["counting"] <= 0.5 and worst.get("ramp", 0.0) <= 0.5


def test_the_modelled_reference_is_the_plain_one_up_to_the_modelled_rounding():
    """MODELS["qsplit"] moves q scale log2 e by at most 2^-16 relative: a score of s nats by s 2^-16, a weight 40 nats below the
    maximum by 40 x 2^-16 = 6e-4 of itself."""
    for shape, shared in (((1, 2, 100, 65, 64), False), ((1, 1, 70, 333, 512), True)):
        for c in AC.cases(shape, shared):
            plain, modelled = AC.reference(c), AC.reference(c, model="qsplit")
            AC.reference(c)
            assert float(((plain - modelled).abs().amax(-1) / c._scale).max()) < 46 * 2.0 ** -16, c.label


def _rejects(c, fmt, tol, fault, kps):
    try:
        AC.check(c, AC.round_to(AC.reference(c, fault=fault, kps=kps), fmt), fmt, tol)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault", sorted(AC.FAULTS), ids=lambda f: f"fault{f}")
def test_every_fault_is_rejected_on_every_route_it_can_occur_on(fault):
    for route in APPLIES[fault]:
        for fmt in AC.route_fmts(route):
            tol = AC.route_tol(route, fmt)
            caught = next((c for c in AC.route_cases(route) if _rejects(c, fmt, tol, fault, _kps(route, c.shape))), None)
            assert caught is not None, f"no case of route {route} [{fmt}] rejects: {AC.FAULTS[fault]}"
            print(f"fault {fault} ({AC.FAULTS[fault]}), {route} [{fmt}]: rejected by {caught.label}")


def test_faults_are_rejected_where_the_families_are_meant_to_see_them():
    """Single-key faults at the lengths where a whole-tensor tolerance lets them pass: 2500 keys, in bf16."""
    shape = (1, 1, 300, 2500, 512)
    tol = AC.TOL16["bf16"]
    cnt, ndl, up = AC.counting(shape), AC.needle(shape), AC.ramp(shape, "up")
    for fault in (1, 2, 3, 4):
        assert _rejects(cnt, "bf16", tol, fault, 288), fault
    for fault in (1, 2, 5, 8):
        assert _rejects(ndl, "bf16", tol, fault, 288), fault
    assert _rejects(cnt, "bf16", tol, 8, 288) and up.family == "ramp"
    # a maximum that rises in tile 1 shows where tile 0 keeps weight in the result: one key more than a tile
    assert _rejects(AC.ramp((1, 1, 100, 33, 512), "up"), "bf16", tol, 9, 0) and _rejects(AC.ramp((1, 2, 100, 65, 64), "up"), "bf16", tol, 9, 0)
    gemm = (1, 1, 300, 2500, 128)
    assert _rejects(AC.counting(gemm), "planes", AC.TOL_SPLIT, 10, 0) and _rejects(AC.ramp(gemm, "saw"), "planes", AC.TOL_SPLIT, 10, 0)
    two = (2, 2, 513, 129, 64)
    for fmt in ("f16", "bf16", "planes"):
        t = AC.TOL_SPLIT if fmt == "planes" else AC.TOL16[fmt]
        assert _rejects(AC.needle(two), fmt, t, 6, 0) and _rejects(AC.counting(two), fmt, t, 6, 0)
        assert _rejects(AC.needle(two), fmt, t, 7, 0) and _rejects(AC.counting(two), fmt, t, 3, 0)
