"""The public switches of the flash caption prefill, walked on the CPU: FastDecoder(prefill=...), PipelineConfig.caption_prefill,
--caption_prefill of both command lines, the way the option reaches get_img_describe / get_img_describe_batch (stubs: no model is
loaded), the C ABI entry points and their ctypes binding, the wrapper's refusal of CPU tensors, and the launch plan."""
import re
import sys
import types
from pathlib import Path

import pytest
import torch

from decoder_stand_in import stand_in_decoder

ROOT = Path(__file__).resolve().parents[1]


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, max_position_embeddings=64)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


def test_fast_decoder_prefill_switch():
    from rsvld_amd import llava_next as LN
    assert LN.FastDecoder.PREFILLS == ("torch", "flash")
    model = _tiny_llama()
    with pytest.raises(ValueError, match="prefill"):
        LN.FastDecoder(model, 32, prefill="x")
    assert LN.FastDecoder(model, 32).prefill == "torch"
    # head_dim 128, g = 2 -- but fp32 on the CPU: the flash prefill raises when the decoder is built, it never falls back to torch
    with pytest.raises(ValueError, match="no fallback"):
        LN.FastDecoder(model, 32, prefill="flash")


def test_default_prefill_on_the_cpu_is_unchanged_by_the_pos0_keyword():
    from rsvld_amd import llava_next as LN
    dec = LN.FastDecoder(_tiny_llama(), 32)
    emb = torch.randn(1, 5, 256, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a = dec.forward(emb, torch.arange(5))
        b = dec.forward(emb, torch.arange(5), pos0=0)
    assert torch.equal(a, b)


def test_pipeline_config_and_command_lines(tmp_path):
    from rsvld_amd import infer, infer_dir
    with pytest.raises(ValueError, match="caption_prefill"):
        infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_prefill="x")
    assert not (tmp_path / "o").exists()
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o")).caption_prefill == "torch"
    assert infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_prefill="flash").caption_prefill == "flash"
    assert infer.build_parser().parse_args(["--input_img", "a.png"]).caption_prefill == "torch"
    assert infer.build_parser().parse_args(["--input_img", "a.png", "--caption_prefill", "flash"]).caption_prefill == "flash"
    assert infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b"]).caption_prefill == "torch"
    assert infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_prefill", "flash"]).caption_prefill == "flash"
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--input_img", "a.png", "--caption_prefill", "sdpa"])
    with pytest.raises(SystemExit):
        infer_dir.build_parser().parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_prefill", "sdpa"])


def test_image_batch_processor_hands_the_option_to_the_pipeline_config(tmp_path):
    from rsvld_amd import infer_dir
    (tmp_path / "in").mkdir()
    proc = infer_dir.ImageBatchProcessor(str(tmp_path / "in"), str(tmp_path / "out"), caption_prefill="flash")
    assert proc.kw["caption_prefill"] == "flash"
    assert infer_dir.ImageBatchProcessor(str(tmp_path / "in"), str(tmp_path / "out")).kw["caption_prefill"] == "torch"


@pytest.mark.parametrize("mode", ["torch", "flash"])
def test_option_reaches_get_img_describe_and_its_batch_form(tmp_path, monkeypatch, mode):
    """The pipeline's two caption calls with stubs in place of the captioner: what arrives as ``decode_prefill``."""
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
    pipe.cfg = infer.PipelineConfig(input_img="a.png", output_dir=str(tmp_path / "o"), caption_prefill=mode, base_model_device="cpu")
    pipe.llava_model = types.SimpleNamespace(config=None)
    pipe.llava_tokenizer = pipe.llava_image_processor = None
    im = Image.new("RGB", (8, 8))
    assert pipe.run_stage2_captioning(im) == "one"
    assert pipe.run_stage2_captioning_batch([im, im]) == ["one", "one"]
    assert seen["single"]["decode_prefill"] == mode and seen["batch"]["decode_prefill"] == mode
    assert seen["single"]["decode_weights"] == "native"


def test_get_img_describe_validates_and_forwards_decode_prefill(monkeypatch):
    from rsvld_amd import llava_next as LN
    with pytest.raises(ValueError, match="decode_prefill"):
        LN.get_img_describe(None, None, None, None, "p", decode_prefill="x")
    with pytest.raises(ValueError, match="decode_prefill"):
        LN.get_img_describe_batch([None], [None], None, None, "p", decode_prefill="x")
    # the decoder of the other mode is rebuilt; the mode reaches FastDecoder
    built = []
    monkeypatch.setattr(LN, "FastDecoder", stand_in_decoder(built, lambda mode: mode.prefill))
    model = types.SimpleNamespace(multimodal_embeds=lambda ids, im, sizes: torch.zeros(1, 7, 4))
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0)
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0)
    assert built == ["torch"]
    LN.caption_tokens_fast(model, None, None, None, 8, False, 1.0, prefill="flash")
    assert built == ["torch", "flash"] and model._fast_decoder.prefill == "flash"
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0, prefill="flash")
    assert built == ["torch", "flash"]
    LN.caption_tokens_fast_batch(model, None, [None], [None], 8, False, 1.0)
    assert built == ["torch", "flash", "torch"]


def test_header_declares_and_lib_binds_the_entry_points():
    from rsvld_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rsvld_hip.h").read_text(), flags=re.S)
    for name in ("rsvld_llama_prefill_attention", "rsvld_plan_llama_prefill_attention"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES
        assert callable(getattr(_lib.load(), name))
    assert len(_lib.SIGNATURES["rsvld_llama_prefill_attention"][1]) == 14
    m = re.search(r"typedef struct rsvld_prefill_attention_plan \{(.*?)\}", src, flags=re.S)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").strip(" ;\n").split(",")]
    assert fields == [f for f, _ in _lib.PrefillAttentionPlan._fields_]


def test_wrapper_refuses_cpu_tensors_and_bad_operands():
    from rsvld_amd import _lib
    from rsvld_amd import prefill_attention as PA
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)
    with pytest.raises(_lib.RsvldError, match="GPU only"):
        PA.llama_prefill_attention(z(4, 8 * 128), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1)
    for bad in (lambda: PA.llama_prefill_attention(z(4, 8 * 128, dt=torch.float32), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1),
                lambda: PA.llama_prefill_attention(z(4, 8 * 128), z(2, 64, 128), z(2, 32, 128), 8, 2, 0.1),
                lambda: PA.llama_prefill_attention(z(4, 7 * 128), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1),
                lambda: PA.llama_prefill_attention(z(4, 8 * 128), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1, pos0=61),
                lambda: PA.llama_prefill_attention(z(4, 8 * 128), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1, pos0=-1),
                lambda: PA.llama_prefill_attention(z(4, 8 * 128), z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1, pos0=torch.tensor(0)),
                lambda: PA.llama_prefill_attention(z(4, 16, 128)[:, ::2], z(2, 64, 128), z(2, 64, 128), 8, 2, 0.1)):
        with pytest.raises(ValueError):
            bad()


def test_plan_is_a_function_of_T_and_the_head_counts_only():
    """128 (position, head-in-group) rows per workgroup, one grid column per kv head; nothing else enters: the entry point takes no
    position and no cache length.  The bench's prompt gives several hundred workgroups."""
    from rsvld_amd import _lib
    from rsvld_amd import prefill_attention as PA
    for T, n_q, n_kv in ((1, 8, 2), (33, 8, 2), (64, 4, 4), (129, 8, 1), (300, 8, 2), (3047, 32, 8), (5, 6, 2)):
        pl = PA.plan(T, n_q, n_kv)
        g = n_q // n_kv
        assert (pl.grid_x, pl.grid_y, pl.rows_per_wg, pl.keys_per_tile) == (-(-T * g // 128), n_kv, 128, 64)
    big = PA.plan(3047, 32, 8)
    assert 256 < big.grid_x * big.grid_y < 1024
    assert _lib.SIGNATURES["rsvld_plan_llama_prefill_attention"][1][:4] == [_lib._i] * 4      # (T, n_q, n_kv, head_dim)
    for args in ((4, 8, 2, 64), (4, 16, 1, 128)):                                               # head_dim 64, g = 16: unsupported
        with pytest.raises(_lib.RsvldError, match="UNSUPPORTED"):
            PA.plan(*args)
    for args in ((0, 8, 2, 128), (4, 8, 3, 128)):
        with pytest.raises(_lib.RsvldError, match="EINVAL"):
            PA.plan(*args)


def test_prefill_attention_kernels_use_no_scratch():
    """Both instantiations are there, with matrix instructions, and the compiler gave them no scratch instruction (a spill would be
    reloaded through the counter the LDS-DMA ring waits on; tools/audit_scratch.py, as tests/test_build_audits.py uses it)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import audit_scratch
    res = audit_scratch.audit("prefill_attention.hip")
    assert len(res) == 2 and all("prefill_attn_d128_kernel" in k for k in res), res
    assert not any(res.values()), res
