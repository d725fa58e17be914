"""The nine non-causal attention kernels of the diffusion and VAE path on exact and adversarial inputs (tests/attention_cases.py;
its premises and the proof that these assertions reject a subtly wrong kernel are in tests/test_attention_cases.py).  Every test
asserts which kernel ran: the library's own plan for the 16-bit launches, the launch names for the rest.

  needle    every element within one spacing of the output format of the target key's V row (a wrong key is off by 1 or more)
  counting  |got - c_d / Nk| <= one spacing, and round(got Nk) == c_d: every key counted once, in its own head and batch
  ramp      per row max_d |got - want| <= tol max_d sum_j p_j |v_jd| against an fp64 softmax; tol = the suite's constant of the route:
            4e-3 / 3e-2 (fp16 / bf16), 2e-5 (fp32), 1e-4 (the split kernels, the GEMM form and attention_f32_split)

(one spacing: the 16-bit type's; 2^-16 relative for planes; 8 x 2^-24 relative for fp32)

Measured maxima of error / bound on an MI355X over every case below (needle: error / one spacing; "=": the needle's result was
bit-equal to the target's V row on every case, which the test then asserts with ``torch.equal``):

    route (kernel)                                    needle          counting        ramp/up, ramp/saw
                                                      fp16   bf16     fp16   bf16     fp16    bf16
    attn_d64b, 4 waves (forced "b"; "c" at Nk <= 64)  =      =        0.49   0.49     0.110   0.123
    attn_d64c (forced "c")                            =      =        0.49   0.49     0.096   0.113
    attn_d64b, 8 waves (16 384 x 77, un-forced)       =      =        0.23   0.22     -       -
    attn_d512b + attn_combine_kernel (k, v separate)  =      =        0.44   0.46     0.121   0.164
    attn_d512d (k is v)                               =      =        0.44   0.46     0.097   0.116
    attn_d512b<shared> ("rows", k is v)               =      =        0.44   0.46     0.097   0.116
    attn_f32_kernel<false>           (fp32)           =               0.063           0.034
    attn_f32_kernel<true>            (fp32)           0.125           0.063           0.025
    attn_split_d64_kernel            (planes)         0.0039          0.19            0.086
    attn_split_d512_kernel           (planes)         0.0039          0.10            0.049
    GEMM form, softmax_rows_split    (planes)         0.0039          0.25            0.064

(0.5 of a 16-bit spacing is the one rounding to the type; the fp32 split kernel and the planes routes miss the needle's V row by
one fp32 rounding of O / l, 2^-24 relative, and are equal where there is one key.)  Every route met its ramp bound against the PLAIN
fp64 softmax: no route needed a modelled reference (attention_cases.ROUTE_MODEL is empty; against MODELS["qsplit"] the two fused
split kernels measure 0.063 / 0.044 instead of 0.086 / 0.049).  No case failed when these tests were first run: no fault was found
in any of the nine kernels."""
import pytest
import torch

import attention_cases as AC
from guarded import LaunchRecorder
from test_gpu_kernels import attn_plan, d64_kernel  # noqa: F401  (d64_kernel: the fixture that forces attn_d64b / attn_d64c)

pytestmark = pytest.mark.gpu

_DT = pytest.mark.parametrize("dtype", AC.DTYPES, ids=AC.DTN.get)
_SID = lambda s: "x".join(str(v) for v in s)
# the routes whose needle result is bit-equal to the target's V row on every case: asserted with torch.equal
NEEDLE_EQUAL = {"d64", "d64_nw8", "d512b", "d512d", "d512b_shared", "f32"}


def _walk(route, fmt, cases, run, kernel=None):
    """Run and check every case; -> {family: worst error / bound}.  Every case is run before the first failure is raised."""
    worst, failures = {}, []
    tol, model = AC.route_tol(route, fmt), AC.ROUTE_MODEL.get(route)
    for c in cases:
        got = AC.unpack(c, run(c))
        try:
            r, equal = AC.check(c, got, fmt, tol, model if c.family == "ramp" else None)
            if c.family == "needle" and route in NEEDLE_EQUAL:
                assert equal, f"{c.label} [{fmt}]: within one spacing of the target's V row, but not bit-equal"
        except AssertionError as e:
            failures.append(str(e))
            r, equal = float("nan"), None
        extra = ""
        if c.family == "ramp" and route in ("split_d64", "split_d512") and bool(torch.isfinite(got).all()):
            extra = " plain %.3g qsplit %.3g" % tuple(float(AC.ramp_ratio(c, got, tol, m)[0].max()) for m in (None, "qsplit"))
        print(f"EXACT {kernel or route} {fmt} {c.family} {r:.3g} {equal}{extra} | {c.label}")
        worst[c.family] = max(worst.get(c.family, 0.0), r)
    assert not failures, "\n".join(failures)
    return worst


def _dev(x64, dtype, cuda):
    return AC.pack(x64).to(dtype).to(cuda)


def _kv(c, dtype, cuda, fused):
    """k, v on the device: two tensors, or column slices of ONE fused k | v tensor (token stride 2 heads D)."""
    if c.shared:
        k = _dev(c.k64, dtype, cuda)
        return k, k
    if not fused:
        return _dev(c.k64, dtype, cuda), _dev(c.v64, dtype, cuda)
    kv = torch.cat([AC.pack(c.k64), AC.pack(c.v64)], -1).to(dtype).to(cuda)
    hd = c.heads * c.D
    return kv[..., :hd], kv[..., hd:]


def _attn16(cuda, c, dtype, fused):
    from rsvld_amd import ops
    k, v = _kv(c, dtype, cuda, fused)
    rec = LaunchRecorder()
    with ops.tuning(profiler=rec):
        got = ops.attention(_dev(c.q64, dtype, cuda), k, v, heads=c.heads, scale=c.scale)
    assert rec.names == [f"attention_d{c.D}" + ("_cross" if c.D == 64 and c.Nk != c.Nq else "")], rec.names
    assert got.dtype == dtype and got.shape == (c.B, c.Nq, c.heads * c.D) and got.is_contiguous()
    return got


@_DT
@pytest.mark.parametrize("shape", AC.D64_SHAPES, ids=_SID)
def test_attention_d64_forced_b_and_c(cuda, shape, dtype, d64_kernel):
    """attn_d64b (4 waves) and attn_d64c, forced: one to five key tiles (attn_d64c requests three in its prologue and rings four), full
    and ragged last tiles, 1 key, Nq on both sides of 128 and 512 rows; forced "c" at Nk <= 64 plans attn_d64b: the plan is asserted.
    k and v are column slices of one fused tensor in every second shape."""
    B, heads, Nq, Nk = shape
    fused = AC.D64_SHAPES.index(shape) % 2 == 1
    ts = (2 if fused else 1) * heads * 64
    name = attn_plan(B, heads, Nq, Nk, 64, tune={"b": 1, "c": 2}[d64_kernel], k_ts=ts, v_ts=ts).name
    assert name == ("d64c" if d64_kernel == "c" and Nk > 64 else "d64b_nw4")
    print(_walk("d64", AC.FMT16[dtype], AC.route_cases("d64", shape + (64,)), lambda c: _attn16(cuda, c, dtype, fused), kernel=name))


@_DT
def test_attention_d64_eight_waves(cuda, dtype):
    """The un-forced route of 16 384 query rows on 77 keys: attn_d64b with 8 waves; needle and counting."""
    B, heads, Nq, Nk = AC.D64_NW8_SHAPE
    assert attn_plan(B, heads, Nq, Nk, 64, k_ts=2 * heads * 64, v_ts=2 * heads * 64).name == "d64b_nw8"
    print(_walk("d64_nw8", AC.FMT16[dtype], AC.route_cases("d64_nw8"), lambda c: _attn16(cuda, c, dtype, True)))


@_DT
@pytest.mark.parametrize("shape", list(AC.D512_SHAPES), ids=_SID)
def test_attention_d512_separate_kv(cuda, shape, dtype):
    """attn_d512b + attn_combine_kernel: 1, 31 .. 33, 95 keys; 600 keys in two ranges (320 + 280), 1024 in four, 2500 in nine (the last
    one ragged).  The needle's targets lie in every range; the ramp's +-a rows make the combine rescale in both directions."""
    B, Nq, Nk = shape
    plan = attn_plan(B, 1, Nq, Nk, 512)
    assert (plan.name, plan.nsplit) == ("d512b", AC.D512_SHAPES[shape])
    print(_walk("d512b", AC.FMT16[dtype], AC.route_cases("d512b", (B, 1, Nq, Nk, 512)), lambda c: _attn16(cuda, c, dtype, False)))


@_DT
@pytest.mark.parametrize("kernel", ["", "rows"], ids=["d512d", "rows"])
@pytest.mark.parametrize("shape", list(AC.D512_SHAPES), ids=_SID)
def test_attention_d512_shared_kv_tile(cuda, shape, kernel, dtype):
    """Keys and values are ONE tensor: attn_d512d (the default) and the row-owning form attn_d512b<shared>, on the same shapes."""
    from rsvld_amd import devtools
    B, Nq, Nk = shape
    route = "d512b_shared" if kernel else "d512d"
    plan = attn_plan(B, 1, Nq, Nk, 512, tune={"": 0, "rows": 4}[kernel], shared=True)
    assert (plan.name, plan.nsplit) == (route, AC.D512_SHAPES[shape])
    try:
        devtools.d512_kernel(kernel)
        print(_walk(route, AC.FMT16[dtype], AC.route_cases(route, (B, 1, Nq, Nk, 512)), lambda c: _attn16(cuda, c, dtype, False)))
    finally:
        devtools.d512_kernel("")


def _attn_f32(cuda, c, split, fused):
    from rsvld_amd import ops
    if fused:
        qkv = torch.cat([AC.pack(x) for x in (c.q64, c.k64, c.v64)], -1).float().to(cuda)
        q, k, v = torch.split(qkv, c.heads * c.D, dim=-1)
    else:
        q, k, v = (_dev(x, torch.float32, cuda) for x in (c.q64, c.k64, c.v64))
    rec = LaunchRecorder()
    with ops.f32_split(ops.SplitPolicy(impl="f32", f16_inputs=()) if split else None), ops.tuning(profiler=rec):
        got = ops.attention(q, k, v, heads=c.heads, scale=c.scale)
    assert rec.names == [f"attention_f32{'_split' if split else ''}_d{c.D}"], rec.names
    assert got.dtype == torch.float32 and got.shape == (c.B, c.Nq, c.heads * c.D)
    return got


@pytest.mark.parametrize("route", ["f32", "f32_split"])
@pytest.mark.parametrize("shape", AC.F32_SHAPES, ids=_SID)
def test_attention_f32_and_its_on_the_fly_split(cuda, shape, route):
    """attn_f32_kernel<false> (rsvld_attention_f32) and attn_f32_kernel<true> (rsvld_attention_f32_split, reached through
    SplitPolicy(impl="f32", f16_inputs=())): D = 64 x 2 heads, 128 and 512; 1, 31 .. 33, 77 and 333 keys; B = 2 once; q | k | v slices
    of one fused tensor once."""
    print(_walk(route, "f32", AC.route_cases(route, shape[:5]), lambda c: _attn_f32(cuda, c, route == "f32_split", shape[5])))


def _planes(cuda, *xs):
    from rsvld_amd import ops
    return [ops.to_planes(_dev(x, torch.float32, cuda)) for x in xs]


def _attn_split_d64(cuda, c, operands):
    from rsvld_amd import ops
    hd = c.heads * c.D
    if operands == "f32":
        q, k, v = (_dev(x, torch.float32, cuda) for x in (c.q64, c.k64, c.v64))
    elif operands == "fused":         # k | v column slices of one planes tensor
        q, = _planes(cuda, c.q64)
        kv = ops.to_planes(torch.cat([AC.pack(c.k64), AC.pack(c.v64)], -1).float().to(cuda))
        k, v = kv[..., :hd], kv[..., hd:]
    else:
        q, k, v = _planes(cuda, c.q64, c.k64, c.v64)
    rec = LaunchRecorder()
    with ops.f32_split(ops.ALL_SPLIT), ops.tuning(profiler=rec):
        got = ops.attention(q, k, v, heads=c.heads, scale=c.scale)
    assert [n for n in rec.names if n != "split_planes"] == ["attention_split_d64" + ("_cross" if c.Nk != c.Nq else "")], rec.names
    assert isinstance(got, ops.Planes) and got.shape == (c.B, c.Nq, hd)
    return got.f32()


@pytest.mark.parametrize("shape", AC.ROUTES["split_d64"]["shapes"], ids=_SID)
def test_attention_split_d64(cuda, shape):
    """attn_split_d64_kernel under ops.ALL_SPLIT on planes (k | v slices of one fused planes tensor in every second shape) and, at
    129 keys, on fp32 operands too: 128 / 129 / 191 / 192 keys sit on both sides of the switch between the steady and the general
    copy of the tile loop; the ramp drives the deferred maximum (``mx > m_run + 8``) and the ``__any(need)`` rescale."""
    i = AC.ROUTES["split_d64"]["shapes"].index(shape)
    print(_walk("split_d64", "planes", AC.route_cases("split_d64", shape), lambda c: _attn_split_d64(cuda, c, "fused" if i % 2 else "planes")))
    if shape[3] == 129:
        print(_walk("split_d64", "planes", AC.route_cases("split_d64", shape), lambda c: _attn_split_d64(cuda, c, "f32")))


def _attn_split_d512(cuda, c):
    from rsvld_amd import ops
    q, x = _planes(cuda, c.q64, c.k64)
    rec = LaunchRecorder()
    with ops.f32_split(ops.ALL_SPLIT), ops.tuning(split_d512_fused_min=1, profiler=rec):
        got = ops.attention(q, x, x, heads=1, scale=c.scale)
    assert rec.names == ["attention_split_d512"], rec.names
    return got.f32()


@pytest.mark.parametrize("shape", AC.ROUTES["split_d512"]["shapes"], ids=_SID)
def test_attention_split_d512_fused(cuda, shape):
    """attn_split_d512_kernel (keys = values = one planes tensor), forced at these sizes by split_d512_fused_min = 1."""
    assert all(c.shared for c in AC.route_cases("split_d512", shape))
    print(_walk("split_d512", "planes", AC.route_cases("split_d512", shape), lambda c: _attn_split_d512(cuda, c)))


def _attn_gemm(cuda, c):
    from rsvld_amd import ops
    q, k, v = _planes(cuda, c.q64, c.k64, c.v64)
    rec = LaunchRecorder()
    with ops.f32_split(ops.ALL_SPLIT), ops.tuning(split_attn_s_bytes=1, split_d512_fused_min=1 << 30, profiler=rec):
        got = ops.attention(q, k, v, heads=1, scale=c.scale)
    blocks = (c.Nq + 255) // 256                                       # rows_blk = 256: two row blocks
    assert rec.names == [f"attention_split_gemm_qk_d{c.D}", "attention_split_softmax", f"attention_split_gemm_pv_d{c.D}"] * blocks and blocks == 2, rec.names
    return got.f32()


@pytest.mark.parametrize("D", AC.GEMM_D)
@pytest.mark.parametrize("Nk", AC.GEMM_NK)
def test_attention_split_gemm_form(cuda, Nk, D):
    """S = Q K^T -> softmax_rows_split_kernel -> P V on the split GEMMs: 0, 1, 3, 4 and 7 pad columns, a second 2048-column pass of
    the softmax's per-thread loops (2049 and 2500 keys), two row blocks."""
    print(_walk("gemm", "planes", AC.route_cases("gemm", (1, 1, AC.GEMM_NQ, Nk, D)), lambda c: _attn_gemm(cuda, c)))
