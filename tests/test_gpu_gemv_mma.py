"""The decode products on MFMAs (``kernel="mfma"`` of ``decode_rows.gemv_rows`` / ``w8.gemv_w8_rows``; csrc/gemv_mma.hip).

Within the mode the contract is bit-identity per row (``torch.equal``: B = 1 through the MFMA entry is the reference), on exactly
computable operands the result is the fp64 sum rounded once, and against the VALU kernels -- the same exact products, summed in fp32
in another order and rounded once to T -- the distance is bounded by
    |mfma - valu| <= ulp_T(|valu|) + 2 K 2^-24 S[b][n],   S = sum_k |W[n][k] x'[b][k]|  (fp64; times scale[n] for e4m3):
the worst-case fp32 summation error of either order (K 2^-24 S each) plus one rounding step of T.  Measured maxima (MI355X, both
dtypes, every shape below): see profiles/caption_decode_mfma_ab.txt."""
import pytest
import torch

from test_gpu_decode_rows import DTYPES, NATIVE_SHAPES, W8_SHAPES, _DTN, _check_rows, _operands

pytestmark = pytest.mark.gpu

# + N < 16 with one K piece; + N = 16 m + 1 on the K-split route (both weight kinds split K = 4 096)
NATIVE = NATIVE_SHAPES + [(5, 8), (33, 4096)]
W8 = W8_SHAPES + [(5, 16), (33, 4096)]
_SID = lambda s: f"{s[0]}x{s[1]}"
# The largest shape of the comparison with the VALU kernels.  The two fp32 sums differ by ~1e-7 relative, so after the rounding to T only
# about one output in a hundred differs: "not everywhere equal" needs thousands of outputs to mean anything (8 x 1 027 here, K-split route,
# N = 16 m + 3, eight rows in two groups).
LARGEST = (1027, 14336)


def _rows_fn(w8_pack, w):
    """-> rows(x [B, K], bias, **kw) through the MFMA entry point of the weight kind."""
    from rsvld_amd import decode_rows as DR
    if w8_pack is not None:
        return lambda a, bias, **kw: DR.gemv_w8_rows(*w8_pack, a, bias, kernel="mfma", **kw)
    return lambda a, bias, **kw: DR.gemv_rows(w, a, bias, kernel="mfma", **kw)


def _single_of(rows):
    """The B = 1 call of the SAME entry point, with ``_check_rows``'s single-row signature."""
    def single(a, bias, **kw):
        if kw.get("residual") is not None:
            kw = dict(kw, residual=kw["residual"][None].contiguous())
        return rows(a[None].contiguous(), bias, **kw)[0]
    return single


def test_the_shapes_cover_both_routes():
    from rsvld_amd import decode_rows as DR
    for shapes, w8 in ((NATIVE, False), (W8, True)):
        routes = {s: DR.plan_gemv_mma(*s, w8=w8).ksplit for s in shapes}
        assert set(routes.values()) == {0, 1}, routes
        assert routes[(33, 4096)] == 1 and routes[(24, 14336)] == 1
        assert DR.plan_gemv_mma(24, 14336, w8=w8).group_rows == 4          # eight rows: two groups, two weight passes


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", NATIVE, ids=_SID)
def test_mfma_rows_are_invariant_to_the_row_count(cuda, dtype, shape):
    w, x, gu, res, b, nw = _operands(cuda, *shape, dtype)
    rows = _rows_fn(None, w)
    _check_rows(_single_of(rows), rows, x, gu, res, b, nw)
    assert torch.equal(rows(x, b), rows(x, b))                                # two runs


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("shape", W8, ids=_SID)
def test_mfma_w8_rows_are_invariant_to_the_row_count(cuda, dtype, shape):
    from rsvld_amd import w8
    w, x, gu, res, b, nw = _operands(cuda, *shape, dtype)
    rows = _rows_fn(w8.pack_rows_e4m3(w), None)
    _check_rows(_single_of(rows), rows, x, gu, res, b, nw)
    assert torch.equal(rows(x, b), rows(x, b))


# ----------------------------------------------------------------------------- exactly computable operands
def _ints(shape, seed):
    return torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("kind", ["native", "e4m3"])
@pytest.mark.parametrize("shape", [(37, 1552), (5, 16), (33, 4096), (24, 14336)], ids=_SID)
def test_integer_operands_are_exact(cuda, dtype, kind, shape):
    """Weights and activations are integers in [-2, 2], bias and residual integers: every product and partial sum is an integer below
    2^24 and |sum| <= 4 K < 65 504, so the fp32 sum is exact in ANY order and the result is the fp64 sum + bias rounded once to T, then
    gv_store's residual step -- for every B, on both routes."""
    from rsvld_amd import decode_rows as DR, w8
    N, K = shape
    wf, xf = _ints((N, K), N + K), _ints((8, K), N + K + 1)
    bias, res = _ints((N,), 3) * 3, _ints((8, N), 4) * 5
    w, x = wf.to(cuda, dtype), xf.to(cuda, dtype)
    if kind == "e4m3":
        q, scale = w8.pack_rows_e4m3(w)
        assert torch.equal(torch.frexp(scale.cpu())[0], torch.full((N,), 0.5)), "scales are powers of two"
        assert torch.equal(w8.dequant(q.cpu(), scale.cpu()), wf)
        rows = _rows_fn((q, scale), None)
        assert DR.plan_gemv_mma(N, K, w8=True).ksplit == (1 if K >= 4096 else 0)
    else:
        rows = _rows_fn(None, w)
        assert DR.plan_gemv_mma(N, K).ksplit == (1 if K >= 4096 else 0)
    s = (xf.double() @ wf.double().T).float()                                     # [8, N], exact
    want = (s + bias).to(dtype)
    want = (res.to(dtype).float() + want.float()).to(dtype)
    for B in range(1, 9):
        got = rows(x[:B].contiguous(), bias.to(cuda, dtype), residual=res[:B].to(cuda, dtype).contiguous())
        assert torch.equal(got.cpu(), want[:B]), (B, float((got.cpu().float() - want[:B].float()).abs().max()))


# ----------------------------------------------------------------------------- against the VALU kernels
def _ulp(v, dtype):
    """Spacing of ``dtype`` at |v| (fp64 tensor): 2^(floor(log2 |v|) - mantissa bits), the subnormal spacing below the normal range."""
    bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.frexp(v.abs().double())[1] - 1                                      # floor(log2 |v|); 0 for v = 0
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - bits)


def _staged(x, nw, eps, dtype):
    """x' of the norm form in torch: T(x rsqrt(mean(x^2) + eps) norm_w), fp32 inside -- only the bound's S is taken from it."""
    xf = x.float()
    return (xf * torch.rsqrt((xf * xf).mean(dim=1, keepdim=True) + eps) * nw.float()).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_DTN.get)
@pytest.mark.parametrize("kind", ["native", "e4m3"])
def test_mfma_against_the_valu_kernel(cuda, dtype, kind):
    from rsvld_amd import decode_rows as DR, w8
    worst, differs_on_largest = 0.0, False
    for shape in (NATIVE if kind == "native" else W8) + [LARGEST]:
        N, K = shape
        w, x, gu, res, b, nw = _operands(cuda, N, K, dtype)
        if kind == "e4m3":
            q, scale = w8.pack_rows_e4m3(w)
            weff = w8.dequant(q.cpu(), scale.cpu()).double()
            call = lambda kernel, **kw: DR.gemv_w8_rows(q, scale, x, kernel=kernel, **kw)
        else:
            weff = w.cpu().double()
            call = lambda kernel, **kw: DR.gemv_rows(w, x, kernel=kernel, **kw)
        for form, kw, xs in (("bias", dict(bias=b), x), ("norm", dict(norm=(nw, 1e-5)), _staged(x, nw, 1e-5, dtype))):
            valu, mfma = call("valu", **kw).cpu().double(), call("mfma", **kw).cpu().double()
            S = xs.cpu().double().abs() @ weff.abs().T                           # [8, N]
            bound = _ulp(valu, dtype) + 2 * K * 2.0 ** -24 * S
            d = (mfma - valu).abs()
            ratio = float((d / bound).max())
            worst = max(worst, ratio)
            print(f"gemv_mma vs valu {kind} {_DTN[dtype]} {N}x{K} {form}: max |d| = {float(d.max()):.3e}, max |d| / bound = {ratio:.3f}, "
                  f"differing elements = {int((d > 0).sum())} of {d.numel()}")
            assert bool((d <= bound).all()), (shape, form, ratio)
            if shape == LARGEST:
                differs_on_largest |= bool((d > 0).any())
    print(f"gemv_mma vs valu {kind} {_DTN[dtype]}: worst |d| / bound = {worst:.3f}")
    assert differs_on_largest, "bit-identical to the VALU kernel on the largest shape: the MFMA path is not what ran"


# ----------------------------------------------------------------------------- operand errors
def test_operand_errors_match_the_valu_wrappers(cuda):
    """Each faulty call raises what the VALU wrapper raises for it, before anything is launched."""
    import guarded
    from rsvld_amd import decode_rows as DR, ops, w8
    f16 = torch.float16
    w = torch.zeros(16, 32, device=cuda, dtype=f16)
    q, scale = w8.pack_rows_e4m3(w)
    x = lambda B: torch.zeros(B, 32, device=cuda, dtype=f16)
    shifted = torch.zeros(3 * 32 + 8, device=cuda, dtype=f16)[4:4 + 96].view(3, 32)   # 8 bytes off a 16-byte boundary
    cases = {
        "B=0": lambda f, k: f(x(0), kernel=k), "B=9": lambda f, k: f(x(9), kernel=k),
        "cpu": lambda f, k: f(x(3).cpu(), kernel=k), "misaligned": lambda f, k: f(shifted, kernel=k),
        "glu+norm": lambda f, k: f(torch.zeros(3, 64, device=cuda, dtype=f16), norm=(torch.ones(64, device=cuda, dtype=f16), 1e-5), glu=True, kernel=k),
        "dtype": lambda f, k: f(x(3).float(), kernel=k),
    }
    for f in (lambda a, **kw: DR.gemv_rows(w, a, **kw), lambda a, **kw: DR.gemv_w8_rows(q, scale, a, **kw)):
        for name, case in cases.items():
            raised = {}
            for k in ("valu", "mfma"):
                rec = guarded.LaunchRecorder()
                with ops.tuning(profiler=rec), pytest.raises(Exception) as e:
                    case(f, k)
                # (a misaligned but contiguous view passes the wrapper's checks; the LIBRARY refuses it -- RSVLD_EINVAL out of gv_check,
                # before any kernel launch -- so the wrapper's ``_launch`` was entered, with either kernel)
                assert rec.names == [] or name == "misaligned", (name, k, rec.names)
                raised[k] = type(e.value)
            assert raised["mfma"] is raised["valu"], (name, raised)
    with pytest.raises(ValueError):
        DR.gemv_rows(w, x(3), kernel="wmma")
