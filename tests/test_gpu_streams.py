"""Which STREAM the work runs on.  The values of every kernel are pinned elsewhere, on the default stream; in production
infer.py issues Stage 2's opening VAE passes on a second, non-blocking stream beside the caption loop, and every wrapper hands
``torch.cuda.current_stream()`` to the library.  A launch that lost that argument would be invisible on the default stream.

* the streamed run of tests/guarded.py (``run_streamed``: every guarded case again on a side stream behind a gate, its operands
  arriving late) is shown to reject what it is for, with torch-only stand-ins: no project kernel is involved;
* ``vae_front`` on a gated side stream, fed a late-arriving image, equals the serial passes bit for bit, and ``just_sampling`` on
  that front equals ``just_sampling`` alone.
(``process()`` with the overlap on and off: test_pipeline_with_live_caption_end_to_end of tests/test_gpu_infer.py.)"""
import os
import sys
import time

import pytest
import torch

import guarded as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import s2_common as S

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- the harness rejects what it is for
def _two_ops(first_stream, second_stream):
    """A two-launch stand-in wrapper: ``tmp = x + 1`` then ``out = tmp * 2``, allocated through ``ops.torch`` as the wrappers do;
    ``*_stream``: None (the current stream, as ``ops._stream()`` would pass) or a zero-argument function returning the stream."""
    from rsvld_amd import ops

    def on(stream, name, work):
        if stream is None:
            return ops._launch(name, 0.0, 0.0, work)
        with torch.cuda.stream(stream()):
            return ops._launch(name, 0.0, 0.0, work)

    def fn(x):
        tmp, out = ops.torch.empty_like(x), ops.torch.empty_like(x)
        on(first_stream, "stand_in_add", lambda: torch.add(x, 1.0, out=tmp))
        on(second_stream, "stand_in_mul", lambda: torch.mul(tmp, 2.0, out=out))
        return out
    return fn


def _x(cuda):
    return torch.randn(257, 96, generator=torch.Generator().manual_seed(0)).to(cuda)


def test_side_stream_is_one_non_default_stream(cuda):
    s = G.side_stream(cuda)
    assert s is G.side_stream(cuda) and s != torch.cuda.default_stream(cuda) and torch.cuda.current_stream(cuda) == torch.cuda.default_stream(cuda)
    gate = G.gate_for(cuda)
    print(f"gate: {gate.ms_per_link:.3f} ms per link")
    assert 0.01 < gate.ms_per_link < 50.0


def test_a_call_wholly_on_the_current_stream_passes(cuda):
    """(c): and the record shows a gate that was pending after both launches."""
    x = _x(cuda)
    got, rec = G.run_guarded(_two_ops(None, None), {"x": x}, expect=("stand_in_add", "stand_in_mul"))
    assert torch.equal(got, (x + 1.0) * 2.0)
    log = rec.streamed
    assert log["conclusive"] and log["names"] == ["stand_in_add", "stand_in_mul"] and log["tries"][-1]["links"] >= 1
    assert G.STREAM_LOG[-1] is log


def test_a_call_on_the_default_stream_is_rejected(cuda):
    """(a): the whole body on the default stream -- where a launch with stream 0 goes -- reads operands that have not arrived.  If
    this passes, side streams do not run beside the default stream here and the streamed run proves nothing."""
    inner = _two_ops(None, None)

    def fn(x):
        with torch.cuda.stream(torch.cuda.default_stream(cuda)):
            return inner(x)
    with pytest.raises(G.GuardError, match="on a gated side stream.*not finite"):
        G.run_guarded(fn, {"x": _x(cuda)})
    assert G.STREAM_LOG[-1]["conclusive"]             # rejected by a verdict, not for want of a gate


def test_a_second_launch_on_the_default_stream_is_rejected(cuda):
    """(b): the first launch is where it belongs; the second does not wait for it and reads a workspace that is still poison."""
    with pytest.raises(G.GuardError, match="on a gated side stream.*not finite"):
        G.run_guarded(_two_ops(None, lambda: torch.cuda.default_stream(cuda)), {"x": _x(cuda)})
    assert G.STREAM_LOG[-1]["conclusive"]


def test_a_first_launch_on_the_default_stream_is_rejected(cuda):
    """The other order: the stray first launch writes its workspace from poisoned operands before the second reads it."""
    with pytest.raises(G.GuardError, match="on a gated side stream"):
        G.run_guarded(_two_ops(lambda: torch.cuda.default_stream(cuda), None), {"x": _x(cuda)})
    assert G.STREAM_LOG[-1]["conclusive"]


def test_a_stray_in_place_update_is_rejected(cuda):
    """A launch on the default stream that only WRITES early (an in-place update of an operand): the late arrival overwrites it."""
    from rsvld_amd import ops

    def fn(acc):
        with torch.cuda.stream(torch.cuda.default_stream(cuda)):
            ops._launch("stand_in_fill", 0.0, 0.0, lambda: acc.fill_(3.0))
        return None
    acc = torch.zeros(64, 8, device=cuda)
    with pytest.raises(G.GuardError, match="depends on what lies around"):
        G.run_guarded(fn, {"acc": G.Op(acc, inplace=True)}, streamed=True)


def test_a_finished_gate_is_inconclusive(cuda):
    """(d): a call that waits for its stream finds the gate finished, on the first attempt and on the one with four times the gate:
    reported as inconclusive -- an AssertionError, not a pass and not a skip -- although every value is right."""
    inner = _two_ops(None, None)

    def fn(x):
        out = inner(x)
        torch.cuda.current_stream(cuda).synchronize()
        return out
    n = len(G.STREAM_LOG)
    with pytest.raises(G.Inconclusive, match="had finished"):
        G.run_guarded(fn, {"x": _x(cuda)})
    log = G.STREAM_LOG[-1]
    assert len(G.STREAM_LOG) == n + 1 and not log["conclusive"] and len(log["tries"]) == 2
    assert log["tries"][1]["links"] >= 3 * log["tries"][0]["links"] >= 3
    assert issubclass(G.Inconclusive, AssertionError) and not issubclass(G.Inconclusive, G.GuardError)
    # no gate at all: the same verdict
    ops_ = {"x": G.Op(_x(cuda))}
    with pytest.raises(G.Inconclusive):
        G.run_streamed(fn, ops_, fn(_x(cuda)), {"x": _x(cuda)}, host_ms=0.0, gate_ms=0.0)


# ----------------------------------------------------------------------------- the VAE front of Stage 2
@pytest.fixture(scope="module")
def model(cuda):
    from oracle import seeded
    from rsvld_amd.sgm.util import instantiate_from_config
    m = instantiate_from_config({"target": "rsvld_amd.models.SR_model.SR_backbone", "params": S.product_params()})
    seeded.seed_module(m, S.WEIGHT_SEED)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():      # zero-initialised output convs would make the control branch a no-op: small seeded weights
        for p_ in m.parameters():
            if p_.dim() >= 2 and float(p_.abs().max()) == 0.0:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.02)
    m.to(cuda).eval()
    yield m
    m.set_precision("bf16", "fp16")


def _rng():
    return torch.get_rng_state(), torch.cuda.get_rng_state()


def _set_rng(state):
    torch.set_rng_state(state[0])
    torch.cuda.set_rng_state(state[1])


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("restoration_scale", [4.0, -1], ids=["restore", "norestore"])
@pytest.mark.parametrize("ae_dtype", ["split", "bf16"])
def test_vae_front_on_a_gated_side_stream_equals_the_serial_passes(model, cuda, ae_dtype, restoration_scale):
    """``vae_front`` as infer.py issues it -- on the side stream, here behind a gate and on an image that arrives behind the gate --
    returns the tensors of the default-stream call, and ``just_sampling`` on that front (after ``wait_stream`` / ``record_stream``, as
    ``run_stage3_refinement`` does) the samples of ``just_sampling`` alone; the global RNG restarts from one state before each,
    because the posterior noise is a CPU draw.  Two serial runs agree first: a mismatch is then a stream finding.
    With the restoration pull off nothing in ``vae_front`` may wait for the stream: the gate is still running when it returns.
    (With it on, the upload of the posterior noise -- a CPU draw, as in the reference -- waits for the passes before it.)"""
    m = model
    m.set_precision(ae_dtype, "fp16")
    lq = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(cuda)
    opt = dict(S.PIPE_OPT, num_steps=2, restoration_scale=restoration_scale)
    torch.manual_seed(11)
    state = _rng()

    def serial_front():
        _set_rng(state)
        return m.vae_front(lq, 1, restoration_scale=restoration_scale)

    def sampling(x, front=None):
        return m.just_sampling(x, ["a river delta"], vae_front=front, **opt)

    a = serial_front()
    t0 = time.perf_counter()
    b = serial_front()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (a[2] is not None) == (restoration_scale > 0)
    for x, y, name in zip(a, b, ("_z", "x_stage1", "z_stage1")):
        _same(x, y, f"serial vs serial: {name}")
    _set_rng(state)
    want = sampling(lq)
    after = _rng()
    _set_rng(state)
    _same(want, sampling(lq), "serial vs serial: samples")
    torch.cuda.synchronize()

    for gate_ms in (G.GATE_MARGIN * host_ms + G.GATE_FLOOR_MS, 4 * (G.GATE_MARGIN * host_ms + G.GATE_FLOOR_MS)):
        late = torch.full_like(lq, float("nan"))
        with G.GatedStream(cuda, gate_ms) as g:
            late.copy_(lq)                               # the image: behind the gate
            _set_rng(state)
            front = m.vae_front(late, 1, restoration_scale=restoration_scale)
            pending = g.pending()
        print(f"vae_front {ae_dtype} restoration_scale {restoration_scale}: gate {g.gate_ms:.2f} ms, host {g.host_ms:.2f} ms "
              f"(serial {host_ms:.2f} ms), gate pending at return: {pending}")
        cur = torch.cuda.current_stream(cuda)
        cur.wait_stream(g.side)
        for t in front:
            if t is not None:
                t.record_stream(cur)
        got = sampling(late, front)
        torch.cuda.synchronize()
        if pending or restoration_scale > 0:
            break
    assert pending or restoration_scale > 0, "inconclusive: the gate had finished before vae_front returned"
    for x, y, name in zip(front, a, ("_z", "x_stage1", "z_stage1")):
        _same(x, y, f"side stream vs serial: {name}")
    _same(got, want, "just_sampling on the side-stream front vs alone")
    now = _rng()
    assert torch.equal(now[0], after[0]) and torch.equal(now[1], after[1])      # the same draws, in the same order
