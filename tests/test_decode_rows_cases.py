"""The batched caption pass without a GPU: ``FastDecoder.generate_batch`` on a CPU Llama (the one-after-another route and its generator
hand-over), the grouping / isolation / generator logic of ``ImageBatchProcessor(caption_batch=N)`` on a stub pipeline, and the argument
errors of the ``decode_rows`` wrappers (their kernels: tests/test_gpu_decode_rows.py)."""
import warnings

import pytest
import torch


# ----------------------------------------------------------------------------- generate_batch on the CPU
@pytest.fixture(scope="module")
def cpu_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=256, rms_norm_eps=1e-5, attention_bias=False)
    torch.manual_seed(5)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    embs = [model.model.embed_tokens(torch.randint(0, 97, (1, n), generator=torch.Generator().manual_seed(n))).detach() for n in (4, 19, 33)]
    return model, embs


def _batch(dec, *a, **kw):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = dec.generate_batch(*a, **kw)
    assert sum("one after another" in str(w.message) for w in seen) == 1      # ONE warning names the route
    return out


def test_generate_batch_on_the_cpu_equals_generate_per_row(cpu_llama):
    from rsvld_amd import llava_next as LN
    model, embs = cpu_llama
    dec1 = LN.FastDecoder(model, 64)
    greedy = [dec1.generate(e, 12) for e in embs]
    sampled = []
    for e, s in zip(embs, (1, 2, 3)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(s)
            sampled.append(dec1.generate(e, 12, do_sample=True, temperature=0.7))
    eos = int(greedy[1][4])
    ended = [dec1.generate(e, 12, eos_token_id=eos) for e in embs]
    assert len(ended[1]) <= 5 and int(ended[1][-1]) == eos

    decb = LN.FastDecoder(model, 64, batch=3)
    assert decb.batch == 3 and decb.k[0].shape[0] == 3 and dec1.k[0].shape[0] == 1
    assert [t.tolist() for t in _batch(decb, embs, 12)] == [t.tolist() for t in greedy]
    state = torch.get_rng_state()
    got = _batch(decb, embs, 12, do_sample=True, temperature=0.7, seeds=[1, 2, 3])
    assert [t.tolist() for t in got] == [t.tolist() for t in sampled]
    assert torch.equal(torch.get_rng_state(), state), "the caller's generator moved"
    assert [t.tolist() for t in _batch(decb, embs, 12, eos_token_id=eos)] == [t.tolist() for t in ended]
    with pytest.raises(ValueError):
        decb.generate_batch(embs + embs, 12)
    with pytest.raises(ValueError):
        decb.generate_batch(embs, 12, do_sample=True, seeds=[1, 2])
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError):
            LN.FastDecoder(model, 64, batch=bad)


def test_row_generator_draws_what_the_forked_default_generator_draws():
    """The mechanism behind ``seeds``: a generator of its own seeded s gives ``torch.multinomial`` the draws the default generator gives
    under ``fork_rng`` + ``manual_seed(s)``."""
    p = torch.softmax(torch.randn(1, 500, generator=torch.Generator().manual_seed(0)), dim=-1)
    for s in (1, 2, 3):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(s)
            want = [int(torch.multinomial(p, 1)) for _ in range(20)]
        g = torch.Generator().manual_seed(s)
        assert [int(torch.multinomial(p, 1, generator=g)) for _ in range(20)] == want


# ----------------------------------------------------------------------------- ImageBatchProcessor on a stub pipeline
class StubPipe:
    """Records the calls; Stage 1 and Stage 2 draw from the default generator (as the real stages do)."""

    def __init__(self, bad_stage1=(), bad_batch=False):
        self.calls, self.bad_stage1, self.bad_batch = [], set(bad_stage1), bad_batch
        self.cfg, self.draws = None, {}

    def process(self):
        self.calls.append(("process", self.cfg.filename))
        sr3 = self.run_stage1_sr3_upscale(self.cfg.input_path)
        return self.run_stage3_refinement(sr3, self.run_stage2_captioning(sr3))

    def run_stage1_sr3_upscale(self, path):
        self.calls.append(("stage1", path.stem))
        if path.stem in self.bad_stage1:
            raise RuntimeError("unreadable image")
        torch.rand(3 + len(path.stem))                    # a different number of draws per image
        self._handoff = ("handoff", path.stem)
        return path.stem

    def run_stage2_captioning(self, sr3):
        self.calls.append(("caption", sr3))
        return f"caption of {sr3}"

    def run_stage2_captioning_batch(self, images):
        self.calls.append(("caption_batch", tuple(images)))
        if self.bad_batch:
            raise RuntimeError("a prompt too long for the cache")
        torch.rand(7)                                     # whatever the pass does to the generator must not reach Stage 2
        return [f"caption of {s}" for s in images]

    def run_stage3_refinement(self, sr3, caption, front=None):
        self.calls.append(("stage2", sr3, caption, self._handoff))
        self.draws[sr3] = torch.rand(4)
        return [self.cfg.output_dir / f"{sr3}_final_0.png"]


def _processor(tmp_path, names, pipe, **kw):
    from rsvld_amd.infer_dir import ImageBatchProcessor
    src = tmp_path / "in"
    src.mkdir(exist_ok=True)
    for n in names:
        (src / f"{n}.png").write_bytes(b"")
    proc = ImageBatchProcessor(str(src), str(tmp_path / "out"), seed=42, no_llava=True, **kw)
    proc.pipe = pipe
    return proc


NAMES = ["a", "bb", "ccc", "dddd", "e", "ff", "ggg"]


def test_caption_batch_1_is_todays_loop(tmp_path):
    pipe = StubPipe()
    done, failed = _processor(tmp_path, NAMES[:3], pipe).run()
    assert [c for c in pipe.calls if c[0] == "process"] == [("process", n) for n in NAMES[:3]]
    assert not any(c[0] == "caption_batch" for c in pipe.calls) and len(done) == 3 and not failed


def test_groups_isolation_and_generator_state(tmp_path):
    ref = StubPipe()
    _processor(tmp_path, NAMES, ref).run()
    pipe = StubPipe()
    done, failed = _processor(tmp_path, NAMES, pipe, caption_batch=3).run()
    assert [c[1] for c in pipe.calls if c[0] == "caption_batch"] == [("a", "bb", "ccc"), ("dddd", "e", "ff")]     # 3 / 3 / 1
    assert [c[1] for c in pipe.calls if c[0] == "caption"] == ["ggg"]
    assert not any(c[0] == "process" for c in pipe.calls) and len(done) == 7 and not failed
    order = [c[0] for c in pipe.calls[:7]]
    assert order == ["stage1"] * 3 + ["caption_batch"] + ["stage2"] * 3
    for c in pipe.calls:
        if c[0] == "stage2":                              # its own caption, its own hand-off
            assert c[2] == f"caption of {c[1]}" and c[3] == ("handoff", c[1])
    for n in NAMES:                                       # Stage 2 drew what it draws in the one-by-one loop
        assert torch.equal(pipe.draws[n], ref.draws[n]), n


def test_a_failing_stage1_leaves_the_group(tmp_path):
    pipe = StubPipe(bad_stage1={"bb"})
    done, failed = _processor(tmp_path, NAMES[:3], pipe, caption_batch=3).run()
    assert [p.stem for p in failed] == ["bb"] and len(done) == 2
    assert [c[1] for c in pipe.calls if c[0] == "caption_batch"] == [("a", "ccc")]


def test_a_failing_batch_caption_degrades_to_single_captions(tmp_path):
    ref = StubPipe()
    _processor(tmp_path, NAMES[:3], ref).run()
    pipe = StubPipe(bad_batch=True)
    done, failed = _processor(tmp_path, NAMES[:3], pipe, caption_batch=3).run()
    assert len(done) == 3 and not failed
    assert [c[1] for c in pipe.calls if c[0] == "caption"] == NAMES[:3]
    for n in NAMES[:3]:
        assert torch.equal(pipe.draws[n], ref.draws[n])


def test_caption_batch_bounds_and_flag():
    from rsvld_amd import infer_dir
    p = infer_dir.build_parser()
    assert p.parse_args(["--image_dir", "a", "--save_dir", "b"]).caption_batch == 1
    assert p.parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_batch", "8"]).caption_batch == 8
    for bad in ("0", "9"):
        with pytest.raises(SystemExit):
            p.parse_args(["--image_dir", "a", "--save_dir", "b", "--caption_batch", bad])


# ----------------------------------------------------------------------------- wrapper contracts
def test_decode_rows_wrappers_check_their_operands():
    from rsvld_amd import _lib, decode_rows as DR
    w = torch.zeros(16, 32, dtype=torch.float16)
    q, scale = torch.zeros(16, 32, dtype=torch.uint8), torch.ones(16)
    x = lambda B, K=32: torch.zeros(B, K, dtype=torch.float16)
    for B in (0, 9):                                      # B outside 1..8
        with pytest.raises(_lib.RsvldOperandError):
            DR.gemv_rows(w, x(B))
        with pytest.raises(_lib.RsvldOperandError):
            DR.gemv_w8_rows(q, scale, x(B))
    with pytest.raises(_lib.RsvldOperandError):
        DR.gemv_rows(w, torch.zeros(32, dtype=torch.float16))                            # one row is [1, K]
    with pytest.raises(_lib.RsvldOperandError):
        DR.gemv_rows(w, x(3), residual=torch.zeros(2, 16, dtype=torch.float16))          # mismatched row counts
    with pytest.raises(_lib.RsvldOperandError):
        DR.gemv_w8_rows(q, scale, x(3), residual=torch.zeros(4, 16, dtype=torch.float16))
    with pytest.raises(_lib.RsvldOperandError):
        DR.gemv_rows(w, x(3, 64))                                                         # 2 K columns without glu
    with pytest.raises(_lib.RsvldOperandError):
        DR.gemv_rows(w, x(2, 64), norm=(torch.zeros(64, dtype=torch.float16), 1e-5), glu=True)
    kc = torch.zeros(3, 2, 64, 128, dtype=torch.float16)
    qkv, cs = torch.zeros(3, 12 * 128, dtype=torch.float16), torch.zeros(3, 128, dtype=torch.float16)
    with pytest.raises(_lib.RsvldOperandError):
        DR.llama_decode_attention_rows(qkv, cs, cs, torch.zeros(2, dtype=torch.int64), kc, kc.clone(), 8, 2, 0.1)     # two positions, three sequences
    with pytest.raises(_lib.RsvldOperandError):
        DR.llama_decode_attention_rows(qkv[:2], cs, cs, torch.zeros(3, dtype=torch.int64), kc, kc.clone(), 8, 2, 0.1)
    big = torch.zeros(9, 2, 64, 128, dtype=torch.float16)
    with pytest.raises(_lib.RsvldOperandError):
        DR.llama_decode_attention_rows(torch.zeros(9, 12 * 128, dtype=torch.float16), torch.zeros(9, 128, dtype=torch.float16),
                                       torch.zeros(9, 128, dtype=torch.float16), torch.zeros(9, dtype=torch.int64), big, big.clone(), 8, 2, 0.1)
    # well-formed operands on the CPU: there is no CPU path
    for call in (lambda: DR.gemv_rows(w, x(3)), lambda: DR.gemv_w8_rows(q, scale, x(3)),
                 lambda: DR.llama_decode_attention_rows(qkv, cs, cs, torch.zeros(3, dtype=torch.int64), kc, kc.clone(), 8, 2, 0.1)):
        with pytest.raises(_lib.RsvldError, match="GPU only"):
            call()


def test_c_abi_rejects_row_counts_outside_1_to_8():
    """The library's own check (no launch happens: the arguments are refused first)."""
    import ctypes as C
    from rsvld_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(4096)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    for B in (0, 9, -1):
        assert lib.rsvld_gemv_rows_fused(p, p, None, None, 0.0, None, 0, p, 4, 16, B, _lib.F16, None) == -1
        assert lib.rsvld_gemv_w8_rows_fused(p, p, p, None, None, 0.0, None, 0, p, 4, 16, B, _lib.F16, None) == -1
        assert lib.rsvld_llama_decode_attention_rows(p, p, p, p, p, p, p, p, 8, 2, 128, 64, B, 0.1, _lib.F16, None) == -1
        assert lib.rsvld_llama_decode_attention_rows_ws_bytes(8, 2, 64, B) == 0
    one = lib.rsvld_llama_decode_attention_ws_bytes(8, 2, 300)
    assert lib.rsvld_llama_decode_attention_rows_ws_bytes(8, 2, 300, 5) == 5 * one
