"""The packed-weight life cycle and the precision record of ``hipnn.HipNet``, on the host, for both kinds of root: the SR3 UNet
(Stage 1) and a VAE encoder (Stage 2).  What is at stake is whether a captured hipGraph points into live memory: ``pack_version``
has to grow whenever the masters move or change and on every change of precision, and the packs of one precision must never be
handed out under another.  Needs neither a GPU nor the kernel library: nothing is packed, a sentinel stands in for a pack."""
import pytest
import torch
from torch import nn

# name -> (compute dtype, pack dtype); SR3's ``set_compute_dtype`` parses these names, the Stage-2 root gets the parsed record
MODES = {"fp16": (torch.float16, None), "w2": (torch.float16, torch.float32), "bf16": (torch.bfloat16, None),
         "fp32": (torch.float32, None), "split": (torch.float32, None)}


def _unet():
    from oracle.sr3_oracle import SR3_CFG as c
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    return UNet(in_channel=c["in_channel"], out_channel=c["out_channel"], inner_channel=c["inner_channel"],
                norm_groups=c["norm_groups"], channel_mults=c["channel_mults"], attn_res=list(c["attn_res"]),
                res_blocks=c["res_blocks"], image_size=c["image_size"])


def _encoder():
    from rsvld_amd.sgm.modules.diffusionmodules.model import Encoder
    return Encoder(ch=32, out_ch=3, ch_mult=(1,), num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=16, z_channels=4)


@pytest.fixture(scope="module", params=["sr3_unet", "vae_encoder"])
def root(request):
    return {"sr3_unet": _unet, "vae_encoder": _encoder}[request.param]()


def _switch(net, name, policy=None):
    from rsvld_amd import ops
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    if isinstance(net, UNet):
        net.set_compute_dtype(name, **({} if policy is None else {"policy": policy}))
    else:
        net.set_precision(*MODES[name], (policy or ops.UNET_POLICY) if name == "split" else None)


def _first_conv(net):
    return next(m for m in net.modules() if isinstance(m, nn.Conv2d))


def test_sr3_unet_is_a_hipnet():
    from rsvld_amd.hipnn import HipNet
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    assert issubclass(UNet, HipNet)
    for name in ("invalidate_packed", "pack_version", "load_state_dict", "_load_from_state_dict", "_apply", "precision_key"):
        assert name not in vars(UNet), f"UNet.{name}: the life cycle has one copy, HipNet's"


def test_pack_version_grows_when_the_masters_move_or_change(root):
    sentinel = object()

    def step(what):
        root._pk["sentinel"] = sentinel
        v = root.pack_version
        what()
        assert root.pack_version > v
        assert "sentinel" not in root._pk and root._pk_other == {}

    step(root.invalidate_packed)
    step(lambda: root.load_state_dict({k: v.clone() for k, v in root.state_dict().items()}))
    parent = nn.Sequential(root)
    step(lambda: parent.load_state_dict({k: v.clone() for k, v in parent.state_dict().items()}))
    step(lambda: parent.to("cpu"))


def test_an_identical_switch_changes_nothing(root):
    from rsvld_amd import ops
    for name, policy in (("fp16", None), ("w2", None), ("split", None), ("split", ops.ALL_SPLIT)):
        _switch(root, name, policy)
        v, k, pk = root.pack_version, root.precision_key(), root._pk
        _switch(root, name, policy)
        assert (root.pack_version, root.precision_key()) == (v, k) and root._pk is pk, name
    _switch(root, "fp16")


def test_packs_are_kept_per_compute_and_pack_dtype(root):
    _switch(root, "fp16")
    root.invalidate_packed()
    sentinel = object()
    root._pk["sentinel"] = sentinel
    seen = {root.pack_version}
    for name in ("w2", "bf16", "fp32", "split"):        # "w2" shares fp16's compute dtype and must not share its packs
        _switch(root, name)
        assert "sentinel" not in root._pk, f"a pack made under fp16 was handed out under {name}"
        assert root.pack_version not in seen, name
        seen.add(root.pack_version)
    _switch(root, "fp16")
    assert root._pk.get("sentinel") is sentinel and root.pack_version not in seen
    _switch(root, "w2")
    root.invalidate_packed()                            # drops the packs of every precision, not only the current one's
    for name in ("fp16", "bf16", "w2"):
        _switch(root, name)
        assert "sentinel" not in root._pk, name
    _switch(root, "fp16")


def test_a_change_of_policy_alone_keeps_the_packs(root):
    from rsvld_amd import ops
    _switch(root, "split")
    sentinel = object()
    root._pk["sentinel"] = sentinel
    v, k = root.pack_version, root.precision_key()
    assert root.split == ops.UNET_POLICY and k == (str(torch.float32), str(torch.float32), ops.UNET_POLICY.key())
    _switch(root, "split", ops.ALL_SPLIT)
    assert root._pk.get("sentinel") is sentinel         # the same fp32 masters, packed the same way
    assert root.pack_version > v and root.precision_key() != k and root.split == ops.ALL_SPLIT
    v = root.pack_version
    _switch(root, "fp32")                               # split -> fp32: the same (compute, pack) pair again
    assert root._pk.get("sentinel") is sentinel and root.pack_version > v and root.split is None
    del root._pk["sentinel"]
    _switch(root, "fp16")


def test_precision_record(root):
    """``pack_dtype`` follows ``compute_dtype`` (also one assigned directly) unless a switch named another one."""
    _switch(root, "w2")
    assert (root.compute_dtype, root.pack_dtype) == (torch.float16, torch.float32)
    assert root.precision_key() == (str(torch.float16), str(torch.float32), None)
    _switch(root, "bf16")
    assert (root.compute_dtype, root.pack_dtype) == (torch.bfloat16, torch.bfloat16)
    _switch(root, "fp16")
    assert root.precision_key() == (str(torch.float16), str(torch.float16), None)


def test_sr3_set_compute_dtype_refusals():
    from rsvld_amd.sr3_model.sr3_modules.unet import UNet
    unet = UNet(in_channel=6, out_channel=3, inner_channel=32, norm_groups=16, channel_mults=(1, 2), attn_res=[8], res_blocks=1,
                image_size=16)
    v = unet.pack_version
    with pytest.raises(TypeError):
        unet.set_compute_dtype("split", policy="all")
    with pytest.raises(ValueError):
        unet.set_compute_dtype("fp8")
    with pytest.raises(ValueError):
        unet.set_compute_dtype(torch.float64)
    assert unet.pack_version == v and unet.precision_key() == (str(torch.float16), str(torch.float16), None)
    unet.set_compute_dtype(torch.bfloat16)              # a torch dtype is a name too
    assert unet.compute_dtype == unet.pack_dtype == torch.bfloat16 and unet.pack_version == v + 1


def test_vae_split_defaults_to_none():
    from rsvld_amd.sgm.models.autoencoder import AutoencoderKL
    assert AutoencoderKL.split is None


def test_packing_a_cpu_parameter_is_an_error(root):
    from rsvld_amd._lib import RsvldError
    root.to("cpu")
    with pytest.raises(RsvldError, match="parameters must be on the GPU"):
        root.pk(_first_conv(root))
    assert root._pk == {}
