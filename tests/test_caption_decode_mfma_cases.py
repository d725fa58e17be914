"""The public switches of the MFMA token loop, walked on the CPU: FastDecoder(decode=...), PipelineConfig.caption_decode,
--caption_decode of both command lines, the way the option reaches get_img_describe / get_img_describe_batch, and the route of the
kernels (rsvld_plan_gemv_mma, host only, on the built library).  The kernels themselves: tests/test_gpu_gemv_mma.py."""
import ctypes
import os
import re
import types

import pytest
import torch

from decoder_stand_in import stand_in_decoder
from test_decode_rows_cases import StubPipe, _processor, cpu_llama   # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_tuple_and_the_defaults(tmp_path):
    import inspect
    from rsvld_amd import decode_rows as DR, infer, infer_dir, llava_next as LN, ops, w8
    assert LN.CAPTION_DECODES == ("valu", "mfma") and LN.FastDecoder.DECODES is LN.CAPTION_DECODES
    assert ops.GEMV_KERNELS == LN.CAPTION_DECODES
    assert (LN.FastDecoder.MAX_BATCH, DR.MAX_ROWS) == (8, 8)
    for f, name in ((LN.FastDecoder.__init__, "decode"), (LN.caption_tokens_fast, "decode"), (LN.caption_tokens_fast_batch, "decode"),
                    (DR.gemv_rows, "kernel"), (w8.gemv_w8_rows, "kernel"), (infer_dir.ImageBatchProcessor.__init__, "caption_decode")):
        assert inspect.signature(f).parameters[name].default == "valu", f
    for f in (LN.get_img_describe, LN.get_img_describe_batch):
        assert inspect.signature(f).parameters["decode_kernel"].default is None            # None = "valu", like its siblings
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o")).caption_decode == "valu"
    assert infer.build_parser().parse_args(["--input_img", "a.png"]).caption_decode == "valu"
    assert infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b"]).caption_decode == "valu"


def test_fast_decoder_validates_decode(cpu_llama):
    from rsvld_amd import llava_next as LN
    model, embs = cpu_llama
    with pytest.raises(ValueError, match="decode"):
        LN.FastDecoder(model, 64, decode="x")
    assert LN.FastDecoder(model, 64).decode == "valu"
    dec = LN.FastDecoder(model, 64, batch=2, decode="mfma")     # a CPU model: the fused step is not available, and the mode says so
    assert dec.decode == "mfma"
    with pytest.raises(RuntimeError, match="mfma"):
        dec.generate(embs[0], 4)
    with pytest.raises(RuntimeError, match="mfma"):
        dec.generate_batch(embs[:2], 4)


def test_pipeline_config_and_both_parsers(tmp_path):
    from rsvld_amd import infer, infer_dir
    with pytest.raises(ValueError, match="caption_decode"):
        infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_decode="x")
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_decode="mfma").caption_decode == "mfma"
    assert infer.build_parser().parse_args(["--input_img", "a.png", "--caption_decode", "mfma"]).caption_decode == "mfma"
    a = infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_decode", "mfma", "--caption_batch", "8",
                                             "--caption_weights", "e4m3-only", "--caption_prefill", "flash"])
    assert (a.caption_decode, a.caption_batch, a.caption_weights, a.caption_prefill) == ("mfma", 8, "e4m3-only", "flash")
    for parser, base in ((infer.build_parser(), ["--input_img", "a.png"]), (infer_dir.build_parser(), ["--image_dir", "a", "--save_dir", "b"])):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--caption_decode", "wmma"])
    with pytest.raises(SystemExit):
        infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_batch", "9"])


def test_image_batch_processor_hands_the_option_on(tmp_path):
    """On the stub pipeline of test_decode_rows_cases.py: the option is in every PipelineConfig the processor builds."""
    from rsvld_amd import infer_dir
    pipe = StubPipe()
    proc = _processor(tmp_path, ["a", "b"], pipe, caption_batch=2, caption_decode="mfma")
    assert proc.kw["caption_decode"] == "mfma"
    (tmp_path / "in2").mkdir()
    assert infer_dir.ImageBatchProcessor(str(tmp_path / "in2"), str(tmp_path / "out2")).kw["caption_decode"] == "valu"
    with pytest.raises(ValueError, match="caption_decode"):
        infer_dir.ImageBatchProcessor(str(tmp_path / "in2"), str(tmp_path / "out3"), caption_decode="x")._process_single_image(tmp_path / "in2" / "a.png")


@pytest.mark.parametrize("mode", ["valu", "mfma"])
def test_option_reaches_get_img_describe_and_its_batch_form(tmp_path, monkeypatch, mode):
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
    pipe.cfg = infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_decode=mode, base_model_device="cpu")
    pipe.llava_model = types.SimpleNamespace(config=None)
    pipe.llava_tokenizer = pipe.llava_image_processor = None
    im = Image.new("RGB", (8, 8))
    assert pipe.run_stage2_captioning(im) == "one"
    assert pipe.run_stage2_captioning_batch([im, im]) == ["one", "one"]
    assert seen["single"]["decode_kernel"] == mode and seen["batch"]["decode_kernel"] == mode


def test_get_img_describe_validates_and_the_mode_reaches_the_decoder(monkeypatch):
    from rsvld_amd import llava_next as LN
    with pytest.raises(ValueError, match="decode_kernel"):
        LN.get_img_describe(None, None, None, None, "p", decode_kernel="x")
    with pytest.raises(ValueError, match="decode_kernel"):
        LN.get_img_describe_batch([None], [None], None, None, "p", decode_kernel="x")
    built = []
    monkeypatch.setattr(LN, "FastDecoder", stand_in_decoder(built, lambda mode: mode.decode))
    model = types.SimpleNamespace(multimodal_embeds=lambda ids, im, sizes: torch.zeros(1, 7, 4))
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0)
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0)
    assert built == ["valu"]
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0, decode="mfma")
    assert built == ["valu", "mfma"] and model._fast_decoder.decode == "mfma"
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0, decode="mfma")
    assert built == ["valu", "mfma"]
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0)
    assert built == ["valu", "mfma", "valu"]


def test_wrappers_validate_kernel_before_anything_else():
    from rsvld_amd import decode_rows as DR, w8
    w, x = torch.zeros(16, 32, dtype=torch.float16), torch.zeros(2, 32, dtype=torch.float16)
    with pytest.raises(ValueError, match="kernel"):
        DR.gemv_rows(w, x, kernel="x")
    with pytest.raises(ValueError, match="kernel"):
        w8.gemv_w8_rows(torch.zeros(16, 32, dtype=torch.uint8), torch.ones(16), x, kernel="x")
    from rsvld_amd import _lib
    for k in ("valu", "mfma"):                                  # the same operand errors with either kernel; a CPU tensor raises
        with pytest.raises(_lib.RsvldOperandError):
            DR.gemv_rows(w, torch.zeros(9, 32, dtype=torch.float16), kernel=k)
        with pytest.raises(_lib.RsvldError):
            DR.gemv_rows(w, x, kernel=k)


# ----------------------------------------------------------------------------- the plan, on the built library
def _plan(N, K, w8, dtype=None):
    from rsvld_amd import _lib
    pl = _lib.GemvMmaPlan()
    rc = _lib.load().rsvld_plan_gemv_mma(N, K, w8, _lib.F16 if dtype is None else dtype, pl)
    return rc, tuple(getattr(pl, f) for f, _ in pl._fields_)


def test_plan_has_no_row_count_and_is_a_function_of_its_arguments():
    from rsvld_amd import _lib
    assert len(_lib.SIGNATURES["rsvld_plan_gemv_mma"][1]) == 5            # N, K, w8, dtype, plan*: no B
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    m = re.search(r"int rsvld_plan_gemv_mma\((.*?)\);", src, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["N", "K", "w8", "dtype", "plan"]
    m = re.search(r"typedef struct rsvld_gemv_mma_plan \{(.*?)\}", src, flags=re.S)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").replace(";", "").split(",")]
    assert fields == [f for f, _ in _lib.GemvMmaPlan._fields_]
    for N, K in ((6144, 4096), (37, 1544), (128256, 4096), (5, 16)):
        for w8 in (0, 1):
            if K % (16 if w8 else 8):
                continue
            first = _plan(N, K, w8)
            assert first[0] == 0
            assert _plan(N, K, w8) == first and _plan(N, K, w8, _lib.BF16) == first      # again, after other calls, in the other dtype
    assert _plan(16, 32, 0, _lib.F32)[0] == -1 and _plan(0, 32, 0)[0] == -1 and _plan(16, 0, 0)[0] == -1
    assert _lib.load().rsvld_plan_gemv_mma(16, 32, 0, _lib.F16, None) == -1


def test_plan_rejects_ragged_k():
    assert _plan(16, 36, 0)[0] == -2 and _plan(16, 40, 0)[0] == 0          # K % 8 for 16-bit weights
    assert _plan(16, 40, 1)[0] == -2 and _plan(16, 48, 1)[0] == 0          # K % 16 for e4m3
    assert _plan(16, 32768, 0)[0] == -2 and _plan(16, 32704, 0)[0] == 0    # K's limit: that of the VALU entry points


def test_plan_routes_of_the_8b_decoder():
    """K split for q|k|v, o_proj and down_proj (256 .. 384 blocks of 16 rows), the row route for gate|up and lm_head; down_proj's eight
    rows go in two groups of four."""
    from rsvld_amd import _lib
    names = [f for f, _ in _lib.GemvMmaPlan._fields_]
    for w8 in (0, 1):
        got = {}
        for name, (N, K) in dict(qkv=(6144, 4096), o=(4096, 4096), gu=(28672, 4096), down=(4096, 14336), head=(128256, 4096)).items():
            rc, pl = _plan(N, K, w8)
            assert rc == 0
            got[name] = dict(zip(names, pl))
        assert [got[n]["ksplit"] for n in ("qkv", "o", "down", "gu", "head")] == [1, 1, 1, 0, 0]
        assert all(p["ways"] == (4 if p["ksplit"] else 1) and p["rows_per_block"] == 16 and p["slab_bytes"] == 8192 for p in got.values())
        assert all(p["step_k"] == (512 if w8 else 256) for p in got.values())
        assert (got["qkv"]["blocks"], got["o"]["blocks"], got["gu"]["blocks"], got["head"]["blocks"]) == (384, 256, 448, 2004)
        assert got["down"]["group_rows"] == 4 and got["qkv"]["group_rows"] == 8
        assert got["down"]["steps_per_way"] * 4 * got["down"]["step_k"] >= 14336


def test_entry_points_return_the_valu_error_codes_for_the_same_faults():
    """No launch is reached: every call fails in gv_check (a non-NULL host pointer is never dereferenced by it)."""
    from rsvld_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)
    for valu, mma, pre in ((lib.rsvld_gemv_rows_fused, lib.rsvld_gemv_mma_rows_fused, (p,)),
                           (lib.rsvld_gemv_w8_rows_fused, lib.rsvld_gemv_w8_mma_rows_fused, (p, p))):
        for x, nw, glu, N, K, B, dt in ((p, None, 0, 4, 16, 0, _lib.F16), (p, None, 0, 4, 16, 9, _lib.F16), (None, None, 0, 4, 16, 1, _lib.F16),
                                        (p, None, 0, 4, 12, 1, _lib.F16), (p, None, 0, 4, 40000, 1, _lib.F16), (odd, None, 0, 4, 16, 1, _lib.F16),
                                        (p, p, 1, 4, 16, 1, _lib.F16), (p, None, 0, 4, 16, 1, _lib.F32), (p, None, 0, 0, 16, 1, _lib.BF16)):
            args = pre + (x, None, nw, 0.0, None, glu, p, N, K, B, dt, None)
            rc = valu(*args)
            assert rc in (-1, -2) and mma(*args) == rc, (N, K, B, dt, rc)


def test_new_symbols_are_declared_bound_and_built():
    from rsvld_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    for name in ("rsvld_gemv_mma_rows_fused", "rsvld_gemv_w8_mma_rows_fused", "rsvld_plan_gemv_mma"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", src)
    for mma, valu in (("rsvld_gemv_mma_rows_fused", "rsvld_gemv_rows_fused"), ("rsvld_gemv_w8_mma_rows_fused", "rsvld_gemv_w8_rows_fused")):
        assert _lib.SIGNATURES[mma] == _lib.SIGNATURES[valu]              # the argument order of the existing pair
    mk = open(os.path.join(ROOT, "remote-sensing-vision-language-diffusion-model_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bgemv_mma\.hip\b", mk, flags=re.M)
