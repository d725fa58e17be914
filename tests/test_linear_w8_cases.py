"""``w8.linear_w8`` and the e4m3-only caption mode, walked on the CPU: the premises of the exact-operand generator the GPU tests use
(``build_exact_rows``, as tests/test_w8_cases.py walks ``build_exact``), the wrapper's operand contract, the switches
(``FastDecoder(prefill_weights=..., release_native=...)``, ``PipelineConfig.caption_weights``, ``--caption_weights`` of both command
lines, the way the value reaches ``get_img_describe`` -- stubs: no model is loaded), the launch plan and the C ABI."""
import functools
import re
import sys
import types
from pathlib import Path

import pytest
import torch

from decoder_stand_in import stand_in_decoder
from test_gpu_w8 import build_exact

ROOT = Path(__file__).resolve().parents[1]
F16, BF16 = torch.float16, torch.bfloat16
EXACT_SHAPES = [(17, 16), (1003, 528), (320, 2064), (512, 1024)]     # (N, K): tests/test_gpu_linear_w8.py says what each is for
EXACT_ROWS = [1, 5, 33, 257]


@functools.lru_cache(maxsize=None)
def build_exact_rows(dtype, N, K, M):
    """``build_exact``'s weights, scales and bias (integers |u| <= 7 times per-row powers of two) against ``M`` activation rows, each with
    at most 16 non-zero small integers (|x| <= 2): first and last element of K, both ends of every K quarter, the rest at random -- another
    pattern in every row.  Every partial sum of the e4m3 integers is then an integer far below 2^24 -- exact in fp32 in ANY order -- and
    the product and product + bias are representable in ``dtype``, so an fp64 reference is the kernel's result bit for bit.
    -> dict(w, q, scale, x [M, K], bias, want={"plain", "bias"} [M, N]); computed once per case and never modified."""
    c = build_exact(dtype, N, K)
    g = torch.Generator().manual_seed(N * 31 + K * 7 + M)
    q4 = K // 4
    forced = sorted({0, K - 1} | {min(max(p, 0), K - 1) for i in range(1, 4) for p in (i * q4 - 1, i * q4)})
    r = torch.rand(M, K, generator=g)
    r[:, forced] = 2.0                                                   # the random positions avoid the forced ones
    rest = r.argsort(dim=1)[:, :16 - len(forced)]
    pos = torch.cat([torch.tensor(forced).expand(M, -1), rest], dim=1)
    val = torch.randint(1, 3, pos.shape, generator=g) * (torch.randint(0, 2, pos.shape, generator=g) * 2 - 1)
    x = torch.zeros(M, K, dtype=torch.float64).scatter_(1, pos, val.double())
    # premises
    assert pos.shape[1] == 16 and all(len(set(p)) == 16 for p in pos.tolist()), "positions collide"
    nz = x != 0
    assert bool((nz.sum(1) == 16).all()) and bool(nz[:, forced].all()) and float(x.abs().max()) <= 2
    assert M == 1 or K == 16 or len({tuple(p) for p in nz.tolist()}) > 1, "the rows share one pattern"
    assert M == 1 or not bool((x == x[0]).all()), "the rows are equal"
    qi = c["q"].view(torch.float8_e4m3fn).float()
    assert torch.equal(qi, qi.round()) and float((x.abs() @ qi.abs().double().T).max()) < 2 ** 24
    unit = c["scale"].double()
    prod = x @ c["w"].double().T                                         # [M, N]
    stages = {"plain": prod, "bias": prod + c["bias"].double()}
    for name, v in stages.items():
        assert torch.equal(v.to(dtype).double(), v), f"{name}: not representable in {dtype}"
        assert torch.equal((v / unit).round(), v / unit), f"{name}: not an integer in the row's unit"
    return dict(w=c["w"], q=c["q"], scale=c["scale"], x=x.to(dtype), bias=c["bias"], want={k: v.to(dtype) for k, v in stages.items()})


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_generator_premises(dtype, shape):
    from rsvld_amd import w8
    N, K = shape
    for M in EXACT_ROWS:
        c = build_exact_rows(dtype, N, K, M)                             # (asserts its own premises)
        assert c["x"].shape == (M, K) and c["want"]["plain"].shape == (M, N) and c["x"].dtype == dtype
        # the reference again from the BYTES, the way the kernel sees the weights
        dq = w8.dequant(c["q"], c["scale"]).double()
        assert torch.equal((c["x"].double() @ dq.T).to(dtype), c["want"]["plain"])
        assert torch.equal((c["x"].double() @ dq.T + c["bias"].double()).to(dtype), c["want"]["bias"])
    assert build_exact_rows(dtype, N, K, 5) is build_exact_rows(dtype, N, K, 5)      # shared, computed once
    assert not torch.equal(build_exact_rows(dtype, N, K, 5)["x"][:1], build_exact_rows(dtype, N, K, 1)["x"])


def test_linear_w8_operand_contract():
    from rsvld_amd import _lib, w8
    N, K, M = 6, 32, 3
    q, s = torch.zeros(N, K, dtype=torch.uint8), torch.ones(N)
    x, b = torch.zeros(M, K, dtype=F16), torch.zeros(N, dtype=F16)
    bad = [lambda: w8.linear_w8(q.to(torch.int8), s, x),                        # q is bytes
           lambda: w8.linear_w8(q, s.double(), x),                              # scale is fp32
           lambda: w8.linear_w8(q, s, x.float()),                               # x is 16-bit
           lambda: w8.linear_w8(q, s, x, b.to(BF16)),                           # bias in x's type
           lambda: w8.linear_w8(torch.zeros(N, 24, dtype=torch.uint8), s, torch.zeros(M, 24, dtype=F16)),     # K % 16
           lambda: w8.linear_w8(q, s, torch.zeros(M, 2 * K, dtype=F16)[:, ::2]),                                # rows not contiguous
           lambda: w8.linear_w8(q, s, torch.zeros(M, 2 * K, dtype=F16)[:, :K]),
           lambda: w8.linear_w8(q.t().contiguous().t(), s, x),
           lambda: w8.linear_w8(q, s[:-1], x),                                  # scale [N]
           lambda: w8.linear_w8(q, s, x, b[:-1]),                               # bias [N]
           lambda: w8.linear_w8(q, s, torch.zeros(M, K + 16, dtype=F16)),       # K of x
           lambda: w8.linear_w8(q, s, torch.zeros(K, dtype=F16)),               # x is [M, K]
           lambda: w8.linear_w8(q, s, torch.zeros(0, K, dtype=F16)),            # no rows
           lambda: w8.linear_w8(q, None, x)]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.RsvldOperandError, match="linear_w8"):
            f()
            pytest.fail(f"case {i} was accepted")
    for bias in (None, b):
        with pytest.raises(_lib.RsvldError, match="GPU only"):
            w8.linear_w8(q, s, x, bias)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, max_position_embeddings=64)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


def test_fast_decoder_switches():
    from rsvld_amd import llava_next as LN
    assert LN.FastDecoder.PREFILL_WEIGHTS == ("native", "e4m3") and LN.FastDecoder.WEIGHTS == ("native", "e4m3")
    model = _tiny_llama()
    before = [p.data_ptr() for p in model.parameters()]
    with pytest.raises(ValueError, match="prefill_weights"):
        LN.FastDecoder(model, 32, prefill_weights="x")
    with pytest.raises(ValueError, match="requires weights='e4m3'"):
        LN.FastDecoder(model, 32, prefill_weights="e4m3")
    with pytest.raises(ValueError, match="requires weights='e4m3'"):
        LN.FastDecoder(model, 32, weights="native", prefill_weights="e4m3", release_native=True)
    with pytest.raises(ValueError, match="release_native"):
        LN.FastDecoder(model, 32, release_native=True)
    with pytest.raises(ValueError, match="release_native"):
        LN.FastDecoder(model, 32, weights="e4m3", release_native=True)
    # fp32 weights on the CPU cannot be packed: the released mode raises BEFORE it releases anything, it never falls back
    with pytest.raises(ValueError, match="no fallback"):
        LN.FastDecoder(model, 32, weights="e4m3", prefill_weights="e4m3", release_native=True)
    assert [p.data_ptr() for p in model.parameters()] == before and all(p.numel() for p in model.parameters())
    assert LN.FastDecoder.PARKED not in model.__dict__
    dec = LN.FastDecoder(model, 32)
    assert (dec.weights, dec.prefill_weights, dec.release_native) == ("native", "native", False)
    assert LN.CAPTION_WEIGHTS == ("native", "e4m3", "e4m3-only")
    assert LN.decoder_mode("native") == dict(weights="native", prefill_weights="native", release_native=False)
    assert LN.decoder_mode("e4m3") == dict(weights="e4m3", prefill_weights="native", release_native=False)
    assert LN.decoder_mode("e4m3-only") == dict(weights="e4m3", prefill_weights="e4m3", release_native=True)
    with pytest.raises(ValueError):
        LN.decoder_mode("int4")


def test_released_model_refuses_whatever_needs_the_16_bit_weights(tmp_path):
    """The parked packs mark the model: the checks come before anything is touched (a stand-in list is enough on the CPU)."""
    from rsvld_amd import llava_next as LN
    model = _tiny_llama()
    model.__dict__[LN.FastDecoder.PARKED] = [None, None]
    for kw in (dict(), dict(weights="e4m3"), dict(weights="native", prefill="torch")):
        with pytest.raises(RuntimeError, match="reload the model"):
            LN.FastDecoder(model, 32, **kw)
    with pytest.raises(RuntimeError, match="reload the model"):
        LN.merge_lora(model, str(tmp_path))
    # ... and packs that no longer match the model (its parameters hold elements) are not adopted
    with pytest.raises(RuntimeError, match="reload the model"):
        LN.FastDecoder(model, 32, weights="e4m3", prefill_weights="e4m3")


def test_pipeline_config_and_command_lines(tmp_path):
    from rsvld_amd import infer, infer_dir, llava_next as LN
    cfg = lambda **kw: infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), **kw)
    for bad in ("x", "int4"):
        with pytest.raises(ValueError, match="caption_weights"):
            cfg(caption_weights=bad)
        with pytest.raises(SystemExit):
            infer.build_parser().parse_args(["--input_img", "a.png", "--caption_weights", bad])
        with pytest.raises(SystemExit):
            infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_weights", bad])
        with pytest.raises(ValueError, match="decode_weights"):
            LN.get_img_describe(None, None, None, None, "p", decode_weights=bad)
        with pytest.raises(ValueError, match="decode_weights"):
            LN.get_img_describe_batch([None], [None], None, None, "p", decode_weights=bad)
    assert not (tmp_path / "o").exists()
    assert cfg().caption_weights == "native"
    assert cfg(caption_weights="e4m3-only").caption_weights == "e4m3-only"
    assert infer.build_parser().parse_args(["--input_img", "a.png"]).caption_weights == "native"
    assert infer.build_parser().parse_args(["--input_img", "a.png", "--caption_weights", "e4m3-only"]).caption_weights == "e4m3-only"
    a = infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_weights", "e4m3-only", "--caption_prefill", "flash",
                                             "--caption_batch", "4"])
    assert (a.caption_weights, a.caption_prefill, a.caption_batch) == ("e4m3-only", "flash", 4)
    assert infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b"]).caption_weights == "native"


def test_value_reaches_get_img_describe_and_the_decoder(tmp_path, monkeypatch):
    """The pipeline's two caption calls with stubs in place of the captioner: what arrives as ``decode_weights``; then, with a stub in
    place of the decoder, the three keywords ``caption_tokens_fast(_batch)`` build it with and compare on the next call."""
    from PIL import Image
    from rsvld_amd import infer, llava_next as LN
    seen = {}
    monkeypatch.setattr(LN, "process_images", lambda imgs, proc, cfg: [torch.zeros(1)])

    def single(**kw):
        seen["single"] = kw
        return ["one"]

    def batch(**kw):
        seen["batch"] = kw
        return ["one"] * len(kw["images"])
    monkeypatch.setattr(LN, "get_img_describe", single)
    monkeypatch.setattr(LN, "get_img_describe_batch", batch)
    pipe = object.__new__(infer.SuperResolutionPipeline)
    pipe.cfg = infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_weights="e4m3-only", base_model_device="cpu")
    pipe.llava_model = types.SimpleNamespace(config=None)
    pipe.llava_tokenizer = pipe.llava_image_processor = None
    im = Image.new("RGB", (8, 8))
    assert pipe.run_stage2_captioning(im) == "one"
    assert pipe.run_stage2_captioning_batch([im, im]) == ["one", "one"]
    assert seen["single"]["decode_weights"] == "e4m3-only" and seen["batch"]["decode_weights"] == "e4m3-only"
    assert seen["single"]["decode_prefill"] == "torch"
    monkeypatch.undo()

    built = []
    monkeypatch.setattr(LN, "FastDecoder", stand_in_decoder(built, lambda mode: (mode.weights, mode.prefill_weights, mode.release_native)))
    model = types.SimpleNamespace(multimodal_embeds=lambda ids, im, sizes: torch.zeros(1, 7, 4))
    only, e4 = ("e4m3", "e4m3", True), ("e4m3", "native", False)
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0, weights="e4m3-only")
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0, weights="e4m3-only")
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0, weights="e4m3-only")
    assert built == [only]
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0, weights="e4m3")       # same ``weights`` field, another mode: rebuilt
    assert built == [only, e4]
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0, weights="e4m3-only")
    assert built == [only, e4, only]


def test_plan_does_not_depend_on_M():
    from rsvld_amd import _lib, w8
    fields = [f for f, _ in _lib.GemmW8Plan._fields_]
    for dtype in (F16, BF16):
        for N, K in ((6144, 4096), (4096, 14336), (28672, 4096), (1003, 528), (17, 16)):
            plans = {M: w8.plan_linear(M, N, K, dtype) for M in (1, 33, 3047)}
            rest = [{f: getattr(p, f) for f in fields if f != "grid_x"} for p in plans.values()]
            assert rest[0] == rest[1] == rest[2], (N, K, rest)
            t = plans[1]
            assert t.tile_m > 0 and t.tile_n > 0 and t.tile_k % 16 == 0 and t.waves > 0
            assert [plans[M].grid_x for M in (1, 33, 3047)] == [-(-M // t.tile_m) for M in (1, 33, 3047)]
            assert t.grid_y == -(-N // t.tile_n)
    with pytest.raises(_lib.RsvldError, match="UNSUPPORTED"):
        w8.plan_linear(4, 8, 24)
    for args in ((0, 8, 16), (4, 0, 16), (4, 8, 0)):
        with pytest.raises(_lib.RsvldError, match="EINVAL"):
            w8.plan_linear(*args)


def test_header_declares_and_lib_binds_the_entry_points():
    from rsvld_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rsvld_hip.h").read_text(), flags=re.S)
    for name in ("rsvld_gemm_w8", "rsvld_plan_gemm_w8"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES
        assert callable(getattr(_lib.load(), name))
    m = re.search(r"int rsvld_gemm_w8\((.*?)\);", src, flags=re.S)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["rsvld_gemm_w8"][1]) == 10
    m = re.search(r"typedef struct rsvld_gemm_w8_plan \{(.*?)\}", src, flags=re.S)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").strip(" ;\n").split(",")]
    assert fields == [f for f, _ in _lib.GemmW8Plan._fields_]


def test_gemm_w8_kernels_use_no_scratch_and_the_unit_is_built():
    sys.path.insert(0, str(ROOT / "tools"))
    import audit_scratch
    assert "gemm_w8.hip" in audit_scratch.UNITS
    res = audit_scratch.audit("gemm_w8.hip")
    assert len(res) == 2 and all("gemm_w8_kernel" in k for k in res), res
    assert not any(res.values()), res
    mk = (ROOT / "remote-sensing-vision-language-diffusion-model_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS\s*:=.*\bgemm_w8\.hip\b", mk, flags=re.M)
