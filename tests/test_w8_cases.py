"""The e4m3 row quantiser's host model (rsvld_amd/w8.py) and the case generators of tests/test_gpu_w8.py, walked on the CPU: the
exponent rule against a brute-force search, idempotence, the error bound, the premises of the exactly computable GEMV operands, and
the public switches of the mode (PipelineConfig.caption_weights, --caption_weights, FastDecoder(weights=...))."""
import pytest
import torch

import test_gpu_w8 as W

DTYPES = W.DTYPES


@pytest.mark.parametrize("dtype", DTYPES, ids=W._DTN.get)
def test_frexp_rule_equals_the_brute_force_search(dtype):
    from rsvld_amd import w8
    w, names = W.edge_rows(dtype, nonfinite=True)
    e = w8.row_exponents_host(w).tolist()
    wf = w.float()
    amax = torch.where(torch.isfinite(wf), wf.abs(), torch.zeros(())).amax(1).double().tolist()
    want = [W.brute_force_exponent(a) for a in amax]
    assert e == want, [(n, a, b) for n, a, b in zip(names, e, want) if a != b]
    # the rows are what their names say: both sides of the 0.875 boundary differ by one, the zero row has e = 0, and the clamp is reached
    for i, n in enumerate(names):
        if n.startswith("448*2^") and n[-1] not in "+-":
            assert names[i + 1] == n + "-" and names[i + 2] == n + "+"
            assert e[i] == e[i + 1] == e[i + 2] - 1 or e[i] == -126, (n, e[i:i + 3])
    assert e[names.index("zero")] == 0
    if dtype == torch.bfloat16:
        assert e[names.index("smallest_subnormal")] == -126            # 2^-133 asks for e = -142: clamped
    q, scale = w8.pack_rows_e4m3_host(w)
    assert scale.dtype == torch.float32 and q.dtype == torch.uint8 and q.shape == w.shape
    assert torch.equal(scale.double(), torch.ldexp(torch.ones(len(e), dtype=torch.float64), torch.tensor(e)))
    # nothing saturates: the largest finite element of every row lands inside e4m3 (no NaN byte except where the weight was not finite)
    assert torch.equal((q & 0x7F) == w8.E4M3_NAN, ~torch.isfinite(wf))


def test_the_cast_rounds_to_nearest_even():
    """What the host model relies on: torch's float8_e4m3fn cast on the CPU."""
    got = torch.tensor([25.0, 27.0, 2.0 ** -10, 3 * 2.0 ** -10, 448.0]).to(torch.float8_e4m3fn).float().tolist()
    assert got == [24.0, 28.0, 0.0, 2.0 ** -8, 448.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=W._DTN.get)
def test_quantising_the_dequantised_rows_returns_them(dtype):
    from rsvld_amd import w8
    w, names = W.edge_rows(dtype, K=64)
    q, scale = w8.pack_rows_e4m3_host(w)
    dq = w8.dequant(q, scale)
    back = dq.to(dtype)
    # dequant is a 16-bit value wherever it is not below the type's own subnormal grid (fp16 rows with e < -15 may hold such)
    ok = torch.equal(back.float(), dq)
    rows = [i for i in range(len(names)) if torch.equal(back[i].float(), dq[i])]
    assert ok or dtype == torch.float16
    assert len(rows) >= len(names) - 6
    q2, s2 = w8.pack_rows_e4m3_host(back[rows])
    q, scale, dq = q[rows], scale[rows], dq[rows]
    assert torch.equal(w8.dequant(q2, s2), dq)                          # the VALUES come back for every row
    # ... and so do (q, scale), with one exception the rule itself makes: an amax that e4m3 rounds DOWN onto 224 = 0.875 x 2^8 (from
    # (224, 232]) is, re-read, an amax with m = 0.875 exactly, which takes the exponent below: the same values as (2 q, scale / 2)
    top = q.view(torch.float8_e4m3fn).float().abs().amax(1)
    same = top != 224
    assert bool(same.any()) and bool((~same).any())                    # (the rows named "448*2^j+" are of the second kind)
    assert torch.equal(q2[same], q[same]) and torch.equal(s2[same], scale[same])
    assert torch.equal(s2[~same] * 2, scale[~same])
    assert torch.equal(q2[~same].view(torch.float8_e4m3fn).float(), q[~same].view(torch.float8_e4m3fn).float() * 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=W._DTN.get)
def test_error_bound(dtype):
    """|dequant - w| <= 2^-4 |w| where |w| >= 2^(e - 6) (e4m3 normals: 3 mantissa bits, half an ulp), <= 2^(e - 10) below (half of the
    subnormal step 2^-9)."""
    from rsvld_amd import w8
    g = torch.Generator().manual_seed(5)
    w = torch.cat([W.edge_rows(dtype, K=64)[0], (torch.randn(64, 64, generator=g) * 0.02).to(dtype)])
    q, scale = w8.pack_rows_e4m3_host(w)
    aw, sc = w.double().abs(), scale.double()[:, None]
    err = (w8.dequant(q, scale).double() - w.double()).abs()
    normal = aw >= sc * 2.0 ** -6
    assert bool(normal.any()) and bool((~normal).any())
    assert bool((err[normal] <= aw[normal] * 2.0 ** -4).all())
    assert bool((err <= sc * 2.0 ** -10)[~normal].all())


@pytest.mark.parametrize("dtype", DTYPES, ids=W._DTN.get)
@pytest.mark.parametrize("shape", W.EXACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_operands_hold_their_premises(dtype, shape):
    c = W.build_exact(dtype, *shape)          # asserts e4m3-exact weights, differing scales, partial sums < 2^24, representable results
    N, K = shape
    assert c["q"].shape == (N, K) and K % 16 == 0
    assert float(c["x"][0]) != 0 and float(c["x"][K - 1]) != 0
    assert not torch.equal(c["want"]["plain"], c["want"]["bias"]) and not torch.equal(c["want"]["bias"], c["want"]["bias_res"])
    # the branch the comments of EXACT_SHAPES name, from the selection rule of rsvld_gemv_w8_fused
    ksplit = K % 64 == 0 and K >= 2048 and (N + 15) // 16 < 1024
    assert ksplit == (shape in ((6, 4096), (6, 14336)))


def test_operand_contracts():
    from rsvld_amd import _lib as L, w8
    with pytest.raises(L.RsvldOperandError):
        w8.pack_rows_e4m3(torch.zeros(4, 24, dtype=torch.float16))             # K % 16
    with pytest.raises(L.RsvldOperandError):
        w8.pack_rows_e4m3(torch.zeros(4, 32, dtype=torch.float32))
    q, s, x = torch.zeros(4, 32, dtype=torch.uint8), torch.ones(4), torch.zeros(32, dtype=torch.float16)
    with pytest.raises(L.RsvldOperandError):
        w8.gemv_w8(q, s.double(), x)
    with pytest.raises(L.RsvldOperandError):
        w8.gemv_w8(q, s, x[:16])
    with pytest.raises(L.RsvldOperandError):
        w8.gemv_w8(q, s, x, residual=torch.zeros(4, dtype=torch.bfloat16))
    with pytest.raises(L.RsvldError, match="GPU only"):                         # a well-formed call on the CPU: there is no CPU path
        w8.gemv_w8(q, s, x)


def test_public_switches(tmp_path):
    from rsvld_amd import infer, infer_dir, llava_next as LN
    with pytest.raises(ValueError, match="caption_weights"):
        infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_weights="x")
    assert not (tmp_path / "o").exists()
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o")).caption_weights == "native"
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_weights="e4m3").caption_weights == "e4m3"
    assert infer.build_parser().parse_args(["--input_img", "a.png"]).caption_weights == "native"
    assert infer.build_parser().parse_args(["--input_img", "a.png", "--caption_weights", "e4m3"]).caption_weights == "e4m3"
    assert infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_weights", "e4m3"]).caption_weights == "e4m3"
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--input_img", "a.png", "--caption_weights", "int4"])
    with pytest.raises(ValueError, match="decode_weights"):
        LN.get_img_describe(None, None, None, None, "p", decode_weights="int4")
    assert LN.FastDecoder.WEIGHTS == ("native", "e4m3")
