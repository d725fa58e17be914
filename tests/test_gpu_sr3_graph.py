"""Stage 1 under hipGraph replay (``GaussianDiffusion.use_graph``, what ``bench.py --workload c2`` measures) against eager runs.

A replay issues the kernels of the captured forward on the values of the current step, and the kernels are deterministic
(test_hand_scheduled_kernels_are_deterministic), so every comparison in this file is ``torch.equal`` on the whole ``continous=True``
stack of kept frames: there is no tolerance here.  Two things are tested:
  * a replayed forward computes what the eager forward computes, in every precision and at the published shape;
  * a capture is never replayed after the state it bakes in has changed (``GaussianDiffusion._graph_key``): precision, policy,
    plan divisor, weights, shape and every launch-context field a wrapper reads at launch time.
No comparison may pass vacuously: two eager runs have to agree first (else a mismatch is a determinism finding, not a graph finding),
and ``unet.forward_nhwc`` is counted -- a capturing pass calls it exactly twice per new key (warm-up + capture), a pure replay pass
never, an eager pass once per step -- together with the number of entries of ``net._graphs``."""
import contextlib

import pytest
import torch

from rsvld_amd import _lib as L
from rsvld_amd import ops

pytestmark = pytest.mark.gpu

WEIGHT_SEED = 1234
STEPS = 4                      # ancestral steps of the small runs: sample_inter = 1, every frame is kept
SCHEDULE = dict(schedule="linear", n_timestep=STEPS, linear_start=1e-6, linear_end=1e-2)


class Case:
    """Seeded conditioning images and noise draws (x_T, then one per step) of one batch shape."""

    def __init__(self, B, H, W, seed, draws=STEPS):
        from oracle import seeded
        self.cond = torch.cat([seeded.synthetic_image((1, 3, H, W), seed=seed + i, smooth=3) for i in range(B)])
        self.noises = [torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed + 100 + i)) for i in range(draws)]


def _run(net, case, graph, sl=slice(None), device="cuda:0"):
    """One ``super_resolution`` of ``case`` (rows ``sl`` of its batch) -> (all kept frames on the host, calls of unet.forward_nhwc)."""
    unet = net.denoise_fn
    calls, forward, draws = [0], unet.forward_nhwc, iter(case.noises)

    def counted(x, level):
        calls[0] += 1
        return forward(x, level)

    unet.forward_nhwc = counted
    net._randn = lambda shape, dev: next(draws)[sl].to(dev)
    net.use_graph = graph
    try:
        out = net.super_resolution(case.cond[sl].to(device), continous=True).cpu()
    finally:
        del unet.forward_nhwc, net._randn
        net.use_graph = False
    return out, calls[0]


def _route(net, case):
    """Names of the launches of one eager sampling run (``LaunchProfiler`` labels: which kernel family every layer went to)."""
    prof = ops.LaunchProfiler()
    with ops.tuning(profiler=prof):
        _run(net, case, False)
    return {r[0] for r in prof.records}


def _reset(net):
    net.denoise_fn.set_compute_dtype("fp16")
    net.batch_invariant, net.use_graph, net._graphs = False, False, {}
    assert ops.context().launch_key() == ops.LaunchContext().launch_key() and ops.context().profiler is None


def _build(cuda):
    """The network of tests/test_gpu_sr3.py's ``sr3`` fixture (oracle SR3_CFG, seeded weights) on a 4-step schedule, plus its state
    dict and a differently seeded one (both on the host, buffers included)."""
    from oracle import seeded, sr3_oracle as O
    from rsvld_amd.sr3_model.sr3_modules.diffusion import GaussianDiffusion
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    c = O.SR3_CFG
    unet = UNet(in_channel=c["in_channel"], out_channel=c["out_channel"], inner_channel=c["inner_channel"],
                norm_groups=c["norm_groups"], channel_mults=c["channel_mults"], attn_res=list(c["attn_res"]),
                res_blocks=c["res_blocks"], dropout=0.2, image_size=c["image_size"])
    net = GaussianDiffusion(unet, image_size=c["image_size"], channels=3, conditional=True)
    seeded.seed_module(net, WEIGHT_SEED)
    net.to(cuda).eval()
    net.set_new_noise_schedule(SCHEDULE, cuda)
    sd_a = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    sd_b = dict(sd_a)
    sd_b.update(seeded.seeded_state_dict([(k, tuple(v.shape)) for k, v in net.named_parameters()], WEIGHT_SEED + 1))
    assert any(not torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    return net, {"a": sd_a, "b": sd_b}


@pytest.fixture(scope="module")
def sr3_net(cuda):
    return _build(cuda)


@pytest.fixture()
def net(sr3_net):
    n = sr3_net[0]
    _reset(n)
    yield n
    _reset(n)


def _cases():
    return {"b2": Case(2, 64, 64, 300), "b3": Case(3, 64, 64, 320), "b1_48x80": Case(1, 48, 80, 340)}


@pytest.fixture(scope="module")
def cases():
    return _cases()


# ------------------------------------------------------------------------------------------------ (a) replay = eager, per precision
@pytest.mark.parametrize("prec", ["fp16", "bf16", "w2", "split", "fp32"])
def test_replay_equals_eager(net, cases, prec):
    """Three passes over batch 2 at 64x64 -- eager, capturing, pure replay -- give the same frames bit for bit."""
    net.denoise_fn.set_compute_dtype(prec)
    case = cases["b2"]
    eager, n = _run(net, case, False)
    assert n == STEPS and eager.shape == ((STEPS + 1) * 2, 3, 64, 64) and bool(torch.isfinite(eager).all())
    again, _ = _run(net, case, False)
    assert torch.equal(eager, again), f"{prec}: two eager runs differ (max|d| = {float((eager - again).abs().max()):.3e})"
    assert not net._graphs
    cap, n = _run(net, case, True)
    assert n == 2 and len(net._graphs) == 1, (n, len(net._graphs))          # one warm-up, one capture, then STEPS replays
    rep, n = _run(net, case, True)
    assert n == 0 and len(net._graphs) == 1, (n, len(net._graphs))          # nothing but replays
    assert torch.equal(cap, eager), f"{prec}: capturing pass vs eager max|d| = {float((cap - eager).abs().max()):.3e}"
    assert torch.equal(rep, eager), f"{prec}: replay pass vs eager max|d| = {float((rep - eager).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ (b) the published shape
@pytest.fixture(scope="module")
def published(cuda):
    """``bench.py --workload c2``: the shipped Stage-1 network, 128 -> 512, batch 4 (three steps of its 50-step schedule)."""
    import bench
    net, _ = bench.build_stage1(50)
    net.batch_invariant = False
    case = Case(4, 512, 512, 400, draws=4)
    case.cond = bench.stage1_input([0, 1, 2, 3], 128, 4)
    yield net, case
    net._graphs = {}


@pytest.mark.parametrize("prec", ["fp16", "w2"])
def test_replay_equals_eager_at_the_published_shape(published, prec):
    """The shape whose number is quoted: halo convolutions, gemm256 and the d = 512 attention with its key split and workspace, all
    allocated inside the capture."""
    from rsvld_amd import measure
    net, case = published
    net.denoise_fn.set_compute_dtype(prec)
    net._graphs = {}
    try:
        with measure.hooks(net, max_steps=3):
            names = _route(net, case)
            assert any(n.startswith("conv_halo") for n in names) and any(n.startswith("gemm_256x256") for n in names) \
                and "attention_d512" in names, sorted(names)
            eager, n = _run(net, case, False)
            # (kept frames of a truncated 50-step loop: the conditioning images and the frame it stopped at, which went through all three steps)
            assert n == 3 and eager.shape == (8, 3, 512, 512) and bool(torch.isfinite(eager).all())
            again, _ = _run(net, case, False)
            assert torch.equal(eager, again), f"{prec}: two eager runs differ"
            cap, n = _run(net, case, True)
            assert n == 2 and len(net._graphs) == 1, (n, len(net._graphs))
            rep, n = _run(net, case, True)
            assert n == 0 and len(net._graphs) == 1, (n, len(net._graphs))
        assert torch.equal(cap, eager), f"{prec}: capturing pass vs eager max|d| = {float((cap - eager).abs().max()):.3e}"
        assert torch.equal(rep, eager), f"{prec}: replay pass vs eager max|d| = {float((rep - eager).abs().max()):.3e}"
    finally:
        net._graphs = {}
        net.denoise_fn.set_compute_dtype("fp16")


# ------------------------------------------------------------------------------------------------ (c) nothing stale is replayed
# One row = (setting A, setting B, inputs of A, inputs of B, expectations).  A setting is a function of the network that applies it and
# returns a context manager (settings that last -- precision, weights -- return a null one).
def _precision(name, policy=None):
    def enter(net):
        net.denoise_fn.set_compute_dtype(name, policy=policy)
        return contextlib.nullcontext()
    return enter


def _context(**fields):
    return lambda net: ops.tuning(**fields)


def _nothing(net):
    return contextlib.nullcontext()


@contextlib.contextmanager
def _batch_invariant(net):
    net.batch_invariant = True
    try:
        yield
    finally:
        net.batch_invariant = False


def _state_dict(which):
    def enter(net):
        net.load_state_dict(STATE[which])
        return contextlib.nullcontext()
    return enter


def _edit(scale):
    """An in-place edit of a packed parameter (the first ResBlock's 3x3 weight) followed by ``invalidate_packed()``."""
    def enter(net):
        unet = net.denoise_fn
        w = unet.downs[1].res_block.block1.block[3].weight
        with torch.no_grad():
            w.copy_(STATE["a"]["denoise_fn.downs.1.res_block.block1.block.3.weight"].to(w.device) * scale)
        unet.invalidate_packed()
        return contextlib.nullcontext()
    return enter


def _round_trip(net):
    dev = net.betas.device
    net.to("cpu")
    net.to(dev)
    return contextlib.nullcontext()


STATE = {}
HALO = lambda names: any(n.startswith("conv_halo") for n in names)       # noqa: E731
PRECS = ("fp16", "w2", "split", "fp32")

# id: (A, B, case of A, case of B, differ, prunes, back, route of A, route of B)
#   differ  do eager A and eager B differ bit for bit?  True: equality of the graph run under B with eager B proves that nothing of A
#           was replayed.  False (bit-identical by design): the proof is the capture count alone.  (Asserted, so that a row cannot
#           quietly stop discriminating.)
#   prunes  the switch bumps ``pack_version``: A's capture is dropped when B's is made (the captures of one version are all that is held)
#   back    what the switch back to A does: "recapture" (a new version again) or "replay" (A's entry is still there and still right)
#   routes  predicates on the eager launch names of A / of B (None: the labels do not show the switch)
ROWS = {}
for _a in PRECS:
    for _b in PRECS:
        if _a != _b:
            # precision_key() tells these apart, and so does pack_version: every set_compute_dtype that changes anything bumps it
            # (fp16 -> w2 -> split -> fp32 -> fp16: 0 to 5), so these rows fail only with BOTH fields out of the key (the round-3 bug:
            # fp32 <-> split toggles replayed the other mode's kernels), and the weight rows below with pack_version alone out of it.
            # (With both out, the pairs that keep the tensor type -- fp16 <-> w2, split <-> fp32 -- and the policy row fail; the other
            # eight pairs are still told apart by the input's dtype.  Neither field is spare.)
            ROWS[f"{_a}->{_b}"] = (_precision(_a), _precision(_b), "b2", "b2", True, True, "recapture", None, None)
ROWS.update({
    "policy": (_precision("split"), _precision("split", ops.SplitPolicy(f16_inputs=())), "b2", "b2", True, True, "recapture",
               lambda n: "attention_d512" in n, lambda n: "attention_split_d512" in n or "attention_split_softmax" in n),
    "batch_invariant": (_nothing, _batch_invariant, "b3", "b3", True, False, "replay", None, None),
    "load_state_dict": (_state_dict("a"), _state_dict("b"), "b2", "b2", True, True, "recapture", None, None),
    "edit+invalidate": (_edit(1.0), _edit(1.25), "b2", "b2", True, True, "recapture", None, None),
    "to(device)": (_nothing, _round_trip, "b2", "b2", False, True, "replay", None, None),
    "shape": (_nothing, _nothing, "b2", "b1_48x80", True, False, "replay", None, None),
    # at 64x64 the default context sends every 3x3 convolution to the gather kernel (fewer than halo_min_wgs = 256 workgroups);
    # halo_min_wgs = 0 sends the eligible ones to the halo kernel, and only there does use_halo = False change anything
    "halo_min_wgs=0": (_nothing, _context(halo_min_wgs=0), "b2", "b2", True, False, "replay", lambda n: not HALO(n), HALO),
    "use_halo=False": (_context(halo_min_wgs=0), _context(halo_min_wgs=0, use_halo=False), "b2", "b2", True, False, "replay",
                       HALO, lambda n: not HALO(n)),
    # the small maps of this network run the K-split implicit GEMM: without it the K loop is summed in another order
    "tune=NO_KSPLIT": (_nothing, _context(tune=L.TUNE_NO_KSPLIT), "b2", "b2", True, False, "replay", None, None),
    # the row-owning form of the shared-tile d = 512 attention against the default head-dimension split: bit-identical by design
    "d512_kernel=rows": (_nothing, _context(d512_kernel=4), "b2", "b2", False, False, "replay",
                         lambda n: "attention_d512" in n, lambda n: "attention_d512" in n),
})


@pytest.mark.parametrize("row", list(ROWS))
def test_nothing_stale_is_replayed(sr3_net, net, cases, row):
    """Capture under A, switch to B, run under graph: equal to eager B, from a NEW capture.  Switch back: equal to eager A again."""
    STATE.update(sr3_net[1])
    enter_a, enter_b, case_a, case_b, differ, prunes, back, route_a, route_b = ROWS[row]
    case_a, case_b = cases[case_a], cases[case_b]
    try:
        with enter_a(net):
            net._graphs = {}
            eager_a, n = _run(net, case_a, False)
            assert n == STEPS
            assert torch.equal(eager_a, _run(net, case_a, False)[0]), "two eager runs under A differ"
            if route_a is not None:
                assert route_a(_route(net, case_a)), "setting A does not take the route this row is about"
            graph_a, n = _run(net, case_a, True)
            assert n == 2 and len(net._graphs) == 1, (n, len(net._graphs))
            assert torch.equal(graph_a, eager_a)
            keys_a = set(net._graphs)
        with enter_b(net):
            eager_b, n = _run(net, case_b, False)
            assert n == STEPS and set(net._graphs) == keys_a
            assert torch.equal(eager_b, _run(net, case_b, False)[0]), "two eager runs under B differ"
            if route_b is not None:
                assert route_b(_route(net, case_b)), "setting B does not take the route this row is about"
            differs = eager_a.shape != eager_b.shape or not torch.equal(eager_a, eager_b)
            print(f"[{row}] eager A and eager B differ bit for bit: {differs}")
            assert differs == differ, "this row's proof (by value / by capture count) is not the one its table entry states"
            graph_b, n = _run(net, case_b, True)
            assert torch.equal(graph_b, eager_b), f"graph run under B vs eager B: max|d| = {float((graph_b - eager_b).abs().max()):.3e} " \
                                                  f"({n} forward calls in that pass; 2 = a new capture, 0 = A's capture replayed)"
            assert n == 2, f"A's capture was replayed under B ({n} forward calls in the first graph pass under B)"
            assert len(net._graphs) == (1 if prunes else 2) and len(set(net._graphs) - keys_a) == 1
            replay_b, n = _run(net, case_b, True)
            assert n == 0 and torch.equal(replay_b, eager_b)
            keys_b = set(net._graphs)
        with enter_a(net):
            graph_a, n = _run(net, case_a, True)
            if back == "recapture":
                assert n == 2 and len(net._graphs) == 1, (n, len(net._graphs))
            else:
                assert n == 0 and set(net._graphs) == keys_b, (n, len(net._graphs))
            assert torch.equal(graph_a, eager_a), f"graph run back under A vs eager A: max|d| = {float((graph_a - eager_a).abs().max()):.3e}"
    finally:
        net._graphs = {}
        if row in ("load_state_dict", "edit+invalidate"):
            net.load_state_dict(STATE["a"])


# ------------------------------------------------------------------------------------------------ (d) batch invariance under replay
def test_batch_invariance_holds_under_replay(net, cases):
    """``batch_invariant`` plans every launch for one image: image b of a replayed batch of 3 is its batch-of-1 run, replayed or eager."""
    case = cases["b3"]
    net.batch_invariant = True
    both, n = _run(net, case, True)
    assert n == 2 and len(net._graphs) == 1
    again, n = _run(net, case, True)
    assert n == 0 and torch.equal(both, again)
    eager3, _ = _run(net, case, False)
    assert torch.equal(both, eager3)
    both = both.view(STEPS + 1, 3, 3, 64, 64)                   # [frame, image, ...]: the stack is frame-major
    for b in range(3):
        one_graph, n = _run(net, case, True, sl=slice(b, b + 1))
        assert n == (2 if b == 0 else 0) and len(net._graphs) == 2, (b, n, len(net._graphs))    # one batch-of-1 capture serves all three
        one_eager, n = _run(net, case, False, sl=slice(b, b + 1))
        assert n == STEPS
        assert torch.equal(one_graph, one_eager), f"image {b}: batch-of-1 replay vs eager"
        assert torch.equal(both[:, b], one_graph), f"image {b}: inside the replayed batch of 3 vs alone: max|d| = " \
                                                    f"{float((both[:, b] - one_graph).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ (e) profiler and graph
def test_profiler_forces_eager_execution(net, cases):
    """A capture would record a LaunchProfiler's events once and a replay none: with a profiler in the context ``use_graph`` runs the
    forward eagerly -- no capture is made or replayed, and every step leaves its records."""
    case = cases["b2"]
    eager, _ = _run(net, case, False)
    p_eager = ops.LaunchProfiler()
    with ops.tuning(profiler=p_eager):
        out, n = _run(net, case, False)
    assert n == STEPS and torch.equal(out, eager) and len(p_eager.records) > STEPS * 50
    p_first = ops.LaunchProfiler()                                   # no capture exists yet: none is made
    with ops.tuning(profiler=p_first):
        out, n = _run(net, case, True)
    assert n == STEPS and not net._graphs and torch.equal(out, eager)
    assert [r[0] for r in p_first.records] == [r[0] for r in p_eager.records]
    cap, n = _run(net, case, True)                                   # a capture exists: it is not replayed under a profiler
    assert n == 2 and len(net._graphs) == 1 and torch.equal(cap, eager)
    p_second = ops.LaunchProfiler()
    with ops.tuning(profiler=p_second):
        out, n = _run(net, case, True)
    assert n == STEPS and len(net._graphs) == 1 and torch.equal(out, eager)
    assert [r[0] for r in p_second.records] == [r[0] for r in p_eager.records]
    sites = sum(1 for r in p_eager.records if r[0] == "attention_d512")
    assert sites > 0 and sites % STEPS == 0                          # every step left its records, not the first one alone
    assert p_second.summary()["attention_d512"]["n"] == sites
    rep, n = _run(net, case, True)                                   # ... and still serves the runs without one
    assert n == 0 and torch.equal(rep, eager)
