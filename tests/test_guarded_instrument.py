"""The guard-band instrument (tests/guarded.py) tested on the CPU: every verdict rejects what it is for -- shown with CPU tensors and
host-side writes through the arena's own raw buffer, no kernel is involved -- and accepts a well-behaved stand-in; the layout the
GPU runs rely on (256-byte aligned payload, flush against the rear guard, derived guard size); the allocation proxy; and the census:
every public wrapper of ops.py that launches a kernel has a guarded case in tests/test_gpu_guarded.py."""
import inspect
import re

import pytest
import torch

import guarded as G
from rsvld_amd import ops


def _raises(fn, *words):
    with pytest.raises(G.GuardError) as e:
        fn()
    for w in words:
        assert w in str(e.value), str(e.value)
    return str(e.value)


# ----------------------------------------------------------------------------- the poison, the layout
def test_poison_byte_is_nan_in_every_operand_type():
    res = G.poison_is_nan()
    assert set(res) == set(G.POISON_DTYPES) | {torch.int32} and all(res.values()), res


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.uint8, torch.int64])
@pytest.mark.parametrize("shape", [(3, 5, 7), (1,), (2, 3, 8, 8), (37, 72)])
def test_placed_tensor_keeps_shape_strides_dtype_alignment_and_ends_flush(dtype, shape):
    a = G.Arena()
    t = (torch.randn(shape) * 10).to(dtype)
    v = a.place(t, "t")
    r = a.regions[0]
    assert v.shape == t.shape and v.stride() == t.stride() and v.dtype == t.dtype and v.is_contiguous()
    assert torch.equal(v, t)
    assert v.data_ptr() % G.ALIGN == 0
    nbytes = t.numel() * t.element_size()
    assert r.end - r.start == nbytes and v.data_ptr() == r.raw.data_ptr() + r.start
    # flush: the byte after the last element and the byte before the first are poison, and the guards are whole
    assert int(r.raw[r.end]) == G.POISON and int(r.raw[r.start - 1]) == G.POISON
    assert r.start >= r.guard and r.raw.numel() - r.end >= r.guard
    assert bool((r.raw[:r.start] == G.POISON).all()) and bool((r.raw[r.end:] == G.POISON).all())
    a.verdict()


def test_guard_size_is_derived_from_the_row_pitch():
    assert G.TILE_ROWS >= 256 and G.MIN_GUARD == 1 << 20
    assert G.guard_bytes(2) == 1 << 20                                   # small rows: the 1 MiB floor
    assert G.guard_bytes(9 * 1024 * 2) == G.TILE_ROWS * 9 * 1024 * 2     # a 3x3 x 1024-channel weight row
    assert G.guard_bytes(4100) % G.ALIGN == 0 and G.guard_bytes(4100) >= G.TILE_ROWS * 4100
    a = G.Arena()
    a.place(torch.zeros(4, 3000, dtype=torch.float32), "wide")            # pitch 12 000 bytes
    a.place(torch.zeros(2, 100, 3 * 2048, dtype=torch.float16)[..., :2048], "slice")   # a column slice: the pitch is the row STRIDE
    assert a.regions[0].guard == G.guard_bytes(12000) and a.regions[1].guard == G.guard_bytes(3 * 2048 * 2)


def test_strided_view_is_placed_with_its_span_or_with_poisoned_gaps():
    qkv = torch.randn(2, 9, 3 * 16).half()
    k = qkv[..., 16:32]
    a = G.Arena()
    kv = a.place(k, "k")                       # with the span it covers: the neighbours' values lie in the gaps
    kp = a.place_view(k, "k (poisoned gaps)")
    for v in (kv, kp):
        assert v.shape == k.shape and v.stride() == k.stride() and v.dtype == k.dtype and torch.equal(v, k)
        assert v.data_ptr() % G.ALIGN == 0
    span = (2 * 9 - 1) * 48 + 16
    r0, r1 = a.regions
    assert r0.end - r0.start == span * 2 == r1.end - r1.start
    assert torch.equal(r0.payload.view(torch.float16), qkv.view(-1)[16:16 + span])
    gaps = r1.is_data == 0
    assert int(gaps.sum()) == (span - k.numel()) * 2 and bool((r1.payload[gaps] == G.POISON).all())
    assert bool(torch.isnan(r1.payload.view(torch.float16)[16:48]).all())       # what a lane that ignores the slice would read
    a.verdict()


# ----------------------------------------------------------------------------- verdict 1: the guards
@pytest.mark.parametrize("where", ["one past the payload", "one before the payload", "first byte of the front guard", "last byte of the rear guard"])
def test_verdict_rejects_a_damaged_guard_byte(where):
    a = G.Arena()
    a.place(torch.randn(5, 24).half(), "x")
    out = a.empty((5, 8), torch.float16, "cpu", name="out")
    out.fill_(1.0)
    a.verdict()
    r = a.regions[1]
    i = {"one past the payload": r.end, "one before the payload": r.start - 1, "first byte of the front guard": 0,
         "last byte of the rear guard": r.raw.numel() - 1}[where]
    r.raw[i] = 0x3C
    side = "rear" if i >= r.end else "front"
    dist = i - r.end + 1 if side == "rear" else r.start - i
    _raises(a.verdict, "guard damaged", "'out'", f"raw byte {i} ", side, f"{dist} byte(s)")
    r.raw[i] = G.POISON
    a.verdict()


def test_a_stand_in_that_overruns_its_output_by_one_row_is_caught():
    """What the instrument is for, with torch as the "kernel": a store one row past a guarded output."""
    a = G.Arena()
    out = a.empty((6, 8), torch.float32, "cpu", name="y")
    r = a.regions[0]
    seven = torch.as_strided(out, (7, 8), (8, 1), out.storage_offset())      # a 7-row view over the 6-row payload: row 6 is guard
    seven.copy_(torch.ones(7, 8))
    msg = _raises(a.verdict, "'y'", "rear guard", "1 byte(s) past")
    assert f"raw byte {r.end} " in msg


# ----------------------------------------------------------------------------- verdict 2: operands
def test_verdict_rejects_an_operand_modified_in_place():
    a = G.Arena()
    x = a.place(torch.arange(40, dtype=torch.float32).view(5, 8), "x")
    a.verdict()
    x[3, 2] += 1.0
    msg = _raises(a.verdict, "operand modified", "'x'", "an element")
    assert int(re.search(r"payload byte (\d+)", msg).group(1)) // 4 == 3 * 8 + 2


def test_inplace_mask_allows_the_documented_elements_only():
    a = G.Arena()
    cache = torch.randn(2, 6, 4).half()
    mask = torch.zeros(2, 6, 4, dtype=torch.bool)
    mask[:, 3] = True                                   # "updated at pos": slot 3 of every head, and only there
    c = a.place(cache, "kcache", inplace=mask)
    c[:, 3] = 7.0
    a.verdict()
    c[1, 4, 0] = 7.0
    msg = _raises(a.verdict, "operand modified", "'kcache'")
    assert int(re.search(r"payload byte (\d+)", msg).group(1)) // 2 == 1 * 24 + 4 * 4
    b = G.Arena()
    acc = b.place(torch.zeros(3, 3), "acc", inplace=True)
    acc += 1
    b.verdict()


def test_verdict_rejects_a_write_into_the_gap_of_a_view():
    a = G.Arena()
    wide = torch.randn(4, 32)
    v = a.place_view(wide[:, 8:16], "rowvec")
    a.verdict()
    r = a.regions[0]
    gap = (8 + 3) * 4                                    # payload byte of element [0, 8 + 3] of the view's row 0: past its 8 columns
    assert int(r.is_data[gap]) == 0 and int(r.is_data[7 * 4]) == 1
    r.raw[r.start + gap] = 0
    _raises(a.verdict, "operand modified", "'rowvec'", "a gap of the view", f"payload byte {gap} ")
    assert torch.equal(v, wide[:, 8:16])


# ----------------------------------------------------------------------------- verdicts 3 and 4: what is returned
def test_verdict_rejects_an_output_element_left_unwritten():
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        a = G.Arena()
        out = a.empty((4, 8), dtype, "cpu")
        out.copy_(torch.randn(4, 8))
        a.verdict(out)
        a.regions[0].payload.view(dtype)[19] = torch.full((1,), G.POISON, dtype=torch.uint8).repeat(dtype.itemsize).view(dtype)[0]
        _raises(lambda: a.verdict(out), "element (2, 3) is not finite", "1 such")
    # an output nobody wrote at all, and the partials riding on a returned tensor
    a = G.Arena()
    out = a.empty((2, 8), torch.float16, "cpu")
    _raises(lambda: a.verdict(out), "element (0, 0)", "16 such")
    out.zero_()
    out._gn_part = (a.empty((1, 2, 8, 2), torch.float32, "cpu"), 2)
    _raises(lambda: a.verdict(out), "result._gn_part")
    out._gn_part[0].zero_()
    a.verdict(out)


def test_verdict_rejects_an_output_that_differs_from_the_plain_run_in_one_bit():
    a = G.Arena()
    plain = torch.randn(3, 8).half()
    out = a.empty((3, 8), torch.float16, "cpu")
    out.copy_(plain)
    a.verdict(out, plain)
    a.regions[0].payload[2 * 13] ^= 1                    # the lowest mantissa bit of element 13
    _raises(lambda: a.verdict(out, plain), "byte 26 (element 13)", "1 bytes differ")
    _raises(lambda: G.same_bits((out, out), (plain,)), "the plain call")
    assert not torch.equal(out, plain) and float((out.float() - plain.float()).abs().max()) < 1e-2


def test_case_supplied_element_test_for_non_float_bytes():
    a = G.Arena()
    rows = a.empty((2, 2, 32), torch.float16, "cpu")       # Q8Rows-like: plane 1 holds e4m3 bytes, 0x7C7C is no fp16 number
    rows[:, 0] = 1.0
    a.regions[0].payload.view(2, 2, 64)[:, 1] = 0x7C
    _raises(lambda: a.verdict(ops.Q8Rows(rows)), "result.t")
    def finite(name, t):
        b = t.view(torch.uint8).view(2, 2, 64)
        return torch.cat([torch.isfinite(t[:, 0]).repeat_interleave(2, -1), (b[:, 1] & 0x7F) != 0x7F], -1)
    a.verdict(ops.Q8Rows(rows), finite=finite)
    a.regions[0].payload.view(2, 2, 64)[1, 1, 5] = 0xFF    # an e4m3 byte left as poison
    _raises(lambda: a.verdict(ops.Q8Rows(rows), finite=finite), "not finite")


# ----------------------------------------------------------------------------- acceptance
def test_a_well_behaved_stand_in_passes_every_verdict():
    g = torch.Generator().manual_seed(0)
    a0, b0 = torch.randn(7, 24, generator=g), torch.randn(7, 24, generator=g)
    arena = G.Arena()
    a, b = arena.place(a0, "a"), arena.place(b0, "b")
    with G.torch_proxy(arena) as T:
        out = T.empty_like(a)
        ws = T.zeros(5, dtype=torch.int32, device="cpu")
    assert bool(torch.isnan(out).all()) and bool((ws == 0).all())          # empty: poison; zeros: the payload only
    torch.add(a, b, out=out)
    arena.verdict(out, a0 + b0)
    assert arena.owns(out) and arena.owns(ws) and not arena.owns(a0)
    assert len(arena.regions) == 4 and [r.kind for r in arena.regions] == ["operand", "operand", "alloc", "alloc"]


def test_run_guarded_end_to_end_with_a_cpu_wrapper(monkeypatch):
    """``run_guarded`` drives a function that allocates through ``ops.torch`` exactly as the wrappers do."""
    def wrapper(x, y, acc):
        out = ops.torch.empty_like(x)
        ops._launch("stand_in [2x3]", 0.0, 0.0, lambda: torch.mul(x, y, out=out))
        acc += 1
        out._nhwc = True
        return out
    g = torch.Generator().manual_seed(1)
    wide = torch.randn(6, 16, generator=g)
    streamed_before = len(G.STREAM_LOG)
    got, rec = G.run_guarded(wrapper, dict(x=torch.randn(6, 8, generator=g), y=G.Op(wide[:, 8:], view=True), acc=G.Op(torch.zeros(3), inplace=True)),
                             expect="stand_in")
    assert rec.names == ["stand_in [2x3]"] and got._nhwc and ops.context().profiler is None and ops.torch is torch
    assert not hasattr(rec, "streamed") and len(G.STREAM_LOG) == streamed_before      # host operands: no side stream, no device is touched
    with pytest.raises(AssertionError, match="did not run"):
        G.run_guarded(wrapper, dict(x=wide, y=wide, acc=G.Op(torch.zeros(3), inplace=True)), expect="stand_in_w2")
    def leaky(x, y):                                                          # reads one row past ``x``: the poison reaches the result
        out = ops.torch.empty_like(x)
        below = torch.as_strided(x, x.shape, x.stride(), x.storage_offset() + x.shape[1])
        return torch.add(x, below * 0.0, out=out)
    with pytest.raises(G.GuardError, match="not finite"):
        G.run_guarded(leaky, dict(x=wide[:5], y=None))        # (outside the guard the row below is ordinary data: invisible)
    def bypass(x):                                                            # an output that did not come from ops.torch
        return x * 2
    with pytest.raises(AssertionError, match="not allocated through"):
        G.run_guarded(bypass, dict(x=wide))


# ----------------------------------------------------------------------------- the proxy
def test_proxy_forwards_everything_else_and_is_restored_after_an_exception():
    arena = G.Arena()
    assert ops.torch is torch
    with pytest.raises(RuntimeError, match="boom"):
        with G.torch_proxy(arena) as T:
            assert ops.torch is T and T is not torch
            assert isinstance(torch.zeros(1), ops.torch.Tensor) and ops.torch.float32 is torch.float32
            assert ops.torch.cuda.current_stream is torch.cuda.current_stream and ops.torch.nn.functional.pad is torch.nn.functional.pad
            e = ops.torch.empty((2, 3, 8), device="cpu", dtype=torch.float16)
            assert e.shape == (2, 3, 8) and e.is_contiguous() and e.data_ptr() % G.ALIGN == 0 and arena.owns(e)
            assert ops.torch.empty(2, 4, dtype=torch.float32, device="cpu").shape == (2, 4)
            z = ops.torch.zeros_like(e, dtype=torch.float32)
            assert z.dtype == torch.float32 and float(z.abs().max()) == 0.0
            e._gn_part, e._nhwc = (z, 3), True                                  # the attributes ops hangs on its outputs
            assert e._gn_part[1] == 3 and e._nhwc
            with pytest.raises(TypeError):
                ops.torch.empty(3, pin_memory=True)
            raise RuntimeError("boom")
    assert ops.torch is torch
    arena.verdict()


def test_packed_weights_are_relocated_slot_by_slot():
    g = torch.Generator().manual_seed(2)
    pc = ops.pack_conv(torch.randn(5, 12, 3, 3, generator=g), torch.randn(5, generator=g), torch.float32, "cpu")
    arena = G.Arena()
    twin = G.copy_packed(pc)
    assert twin.w is pc.w and twin.w2 is None
    ops._w1(twin)
    G.relocate(twin, arena, "pc")
    assert [r.name for r in arena.regions] == ["pc.w", "pc.bias", "pc.w1"]
    for slot in ("w", "bias", "w1"):
        t = getattr(twin, slot)
        assert arena.owns(t) and t.data_ptr() % G.ALIGN == 0
    assert torch.equal(twin.w, pc.w) and twin.w.shape == (8, 9 * 16) and torch.equal(twin.w1, pc.w.half()) and pc.w1 is None
    assert arena.regions[0].guard == G.guard_bytes(9 * 16 * 4)
    n = len(arena.regions)
    G.relocate(twin, arena)                              # already inside: nothing moves
    assert len(arena.regions) == n
    arena.verdict()


# ----------------------------------------------------------------------------- census
# public functions of ops.py that launch nothing: context plumbing, policy queries and the host-side weight re-layout
NO_LAUNCH = {"pad8", "context", "tuning", "set_defaults", "plan_units", "f32_split", "precision_token", "f16_group", "q8_group",
             "set_profiler", "pack_conv"}


def _launching_wrappers():
    """Public functions of ops.py whose source contains ``L.load()`` / ``L.check(``, or that call a function or method that does
    (``maybe_planes`` -> ``to_planes``, ``as_f32`` -> ``Planes.f32``, ``linear`` -> ``conv2d``)."""
    src = {}
    for name, fn in vars(ops).items():
        if inspect.isfunction(fn) and fn.__module__ == ops.__name__:
            src[name] = inspect.getsource(fn)
        elif inspect.isclass(fn) and fn.__module__ == ops.__name__:
            for m, f in vars(fn).items():
                if inspect.isfunction(f) and not m.startswith("__"):
                    src.setdefault(m, inspect.getsource(f))
    launches = {n for n, s in src.items() if "L.load()" in s or "L.check(" in s}
    grew = True
    while grew:
        grew = False
        for n, s in src.items():
            if n not in launches and any(re.search(r"(?<![\w])" + re.escape(c) + r"\(", s) for c in launches):
                launches.add(n)
                grew = True
    public = {n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")}
    return public & launches, public


def test_census_every_launching_wrapper_has_a_guarded_case():
    import test_gpu_guarded as T
    launching, public = _launching_wrappers()
    assert {"conv2d", "linear", "attention", "group_norm", "gemv", "to_planes", "as_f32", "maybe_planes", "adain", "sinusoidal"} <= launching
    assert not (launching & NO_LAUNCH), launching & NO_LAUNCH
    assert public - launching == NO_LAUNCH, (public - launching) ^ NO_LAUNCH      # a new public function is a wrapper or is listed here
    declared = T.declared_wrappers()
    assert declared <= launching, declared - launching                            # no case names something that does not exist
    missing = launching - declared
    assert not missing, f"ops wrappers without a guarded case in tests/test_gpu_guarded.py: {sorted(missing)}"
    # every family of the case tables has its test function, and every case a unique id within it
    for fam, cases in T.FAMILIES.items():
        assert hasattr(T, "test_guarded_" + fam), fam
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
