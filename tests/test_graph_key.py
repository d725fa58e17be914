"""The key of a captured Stage-1 UNet forward (``GaussianDiffusion._graph_key``), on the host: the key has to change with everything
a capture bakes in -- every ``LaunchContext`` field a wrapper reads at launch time, the precision, the packed weights' version, the
input's shape / dtype / device -- or a replay silently runs the launches of another setting (tests/test_gpu_sr3_graph.py shows the
same on the GPU, by value)."""
import pytest
import torch

# another legal value for every LaunchContext field (``_other``: the default must differ from it)
IN_KEY = {"plan_div": 3, "policy": "policy", "tune": 1 << 6, "use_halo": False, "halo_min_wgs": 0, "split_halo_min_wgs": 0,
          "split_d512_fused_min": 64, "split_attn_s_bytes": 1 << 20, "d64_kernel": 2, "d512_kernel": 5}
NOT_IN_KEY = {"profiler": "profiler", "profile_detail": True}     # they bracket and name launches; they do not choose them


def _other(field):
    from rsvld_amd import ops
    v = {**IN_KEY, **NOT_IN_KEY}[field]
    return {"policy": ops.ALL_SPLIT, "profiler": ops.LaunchProfiler()}.get(v, v) if isinstance(v, str) else v


@pytest.fixture()
def net():
    from rsvld_amd.sr3_model.sr3_modules.diffusion import GaussianDiffusion
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    unet = UNet(in_channel=6, out_channel=3, inner_channel=32, norm_groups=16, channel_mults=(1, 2), attn_res=[8], res_blocks=1,
                image_size=16)
    return GaussianDiffusion(unet, image_size=16, channels=3, conditional=True)


def _key(net, shape=(2, 64, 64, 8), dtype=torch.float16, index=0):
    return net._graph_key(shape, dtype, index)


def test_every_launch_context_slot_is_classified():
    """A field added to LaunchContext later has to be put in one of the two lists (and so in or out of the key) by hand."""
    from rsvld_amd import ops
    slots = set(ops.LaunchContext.__slots__)
    assert not (set(IN_KEY) & set(NOT_IN_KEY))
    assert slots - set(IN_KEY) - set(NOT_IN_KEY) == set(), "LaunchContext fields neither in the capture key nor exempt from it"
    assert (set(IN_KEY) | set(NOT_IN_KEY)) - slots == set(), "stale entries: not LaunchContext fields"
    assert set(ops.LaunchContext.NOT_IN_LAUNCH_KEY) == set(NOT_IN_KEY)
    for f in slots:
        assert getattr(ops.LaunchContext(), f) != _other(f), f         # the sweep below really changes the field


@pytest.mark.parametrize("field", sorted(IN_KEY))
def test_launch_context_field_changes_the_key(net, field):
    from rsvld_amd import ops
    base = _key(net)
    with ops.tuning(**{field: _other(field)}):
        assert getattr(ops.context(), field) == _other(field)
        inside = _key(net)
        assert inside != base, f"a capture made under another {field} would be replayed"
        assert ops.context().launch_key() != ops.LaunchContext().launch_key()
    assert _key(net) == base


@pytest.mark.parametrize("field", sorted(NOT_IN_KEY))
def test_profiler_fields_do_not_change_the_key(net, field):
    from rsvld_amd import ops
    base = _key(net)
    with ops.tuning(**{field: _other(field)}):
        assert _key(net) == base
        assert ops.context().launch_key() == ops.LaunchContext().launch_key()


def test_launch_key_is_hashable_and_equal_for_equal_contexts():
    from rsvld_amd import ops
    a = ops.LaunchContext(policy=ops.SplitPolicy(), tune=3)
    b = ops.LaunchContext(policy=ops.SplitPolicy(), tune=3, profile_detail=True)     # an equal policy, another object
    assert a.launch_key() == b.launch_key() and hash(a.launch_key()) == hash(b.launch_key())
    assert a.launch_key() != a.replace(policy=ops.ALL_SPLIT).launch_key()


def test_key_changes_with_every_precision_switch(net):
    from rsvld_amd import ops
    unet = net.denoise_fn
    modes = {"fp16": {}, "w2": {}, "bf16": {}, "split": {}, "fp32": {}, "split/all": {"policy": ops.ALL_SPLIT}}
    keys = {}
    for name, kw in modes.items():
        unet.set_compute_dtype(name.split("/")[0], **kw)
        keys[name] = (_key(net), unet.precision_key())
    assert len({k for k, _ in keys.values()}) == len(modes)
    assert len({p for _, p in keys.values()}) == len(modes)         # told apart by precision_key() alone too, not only by pack_version
    for a in modes:
        for b in modes:
            if a == b:
                continue
            unet.set_compute_dtype(a.split("/")[0], **modes[a])
            ka, va = _key(net), unet.pack_version
            unet.set_compute_dtype(b.split("/")[0], **modes[b])
            assert _key(net) != ka, f"{a} -> {b}"
            assert unet.pack_version > va, f"{a} -> {b}: captures of {a} have to be dropped (they pin its packed weights)"
    unet.set_compute_dtype("fp16")
    v = unet.pack_version
    k = _key(net)
    unet.set_compute_dtype("fp16")                                      # no change: no new version, the same key
    assert unet.pack_version == v and _key(net) == k


def test_key_changes_with_weights_shape_dtype_device(net):
    unet = net.denoise_fn
    base = _key(net)
    assert _key(net) == base                                            # nothing changed
    assert _key(net, shape=(1, 64, 64, 8)) != base and _key(net, shape=(2, 48, 80, 8)) != base
    assert _key(net, shape=torch.Size((2, 64, 64, 8))) == base          # a torch.Size and a tuple name the same shape
    assert _key(net, dtype=torch.bfloat16) != base
    assert _key(net, index=1) != base
    unet.invalidate_packed()
    k1 = _key(net)
    assert k1 != base
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    k2 = _key(net)
    assert k2 not in (base, k1)
    unet.load_state_dict({k: v.clone() for k, v in unet.state_dict().items()})
    k3 = _key(net)
    assert k3 not in (base, k1, k2)
    net.to("cpu")                                                       # any _apply may move the masters the graph points into
    assert _key(net) not in (base, k1, k2, k3)


def test_key_holds_the_pack_version_where_the_pruning_reads_it(net):
    """``_unet_eps`` drops the captures whose ``key[3]`` is an older pack_version."""
    net.denoise_fn.invalidate_packed()
    assert _key(net)[3] == net.denoise_fn.pack_version
