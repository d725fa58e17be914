"""The split precision's policies (rsvld_amd.ops.SplitPolicy) through the package's own ResBlock (sgm/modules/diffusionmodules/
openaimodel.py): the policy names a route for each of the block's two 3x3 convolutions ("conv1", "conv2"), the block labels its
convolutions, ``ops._conv2d_split`` turns label + policy into a kernel.  The per-layer tests (test_gpu_split.py) pass the label by
hand; here the labels come from the model, so swapped labels, a dropped label or a routing branch that reads the wrong group show.

* Route matrix: for every policy, the launches of conv1's and of conv2's shape are the kernels the policy names for that group --
  ``conv_halo_128_q8`` behind ``groupnorm_apply_q8`` (q8_convs, where eligible), the weight-pair form ``*_w2`` (f16_inputs), the three-MFMA
  split form ``*_split`` (else), ``conv_f32`` (no policy) -- against the block in float64, and bit-identical when run twice.
* Census: in a reduced-depth UNet and ControlNet with SDXL channel widths, the number of ``conv_halo_128_q8`` launches is the number of
  ResBlock convolutions ``_q8_conv_eligible`` accepts (both groups, and each group alone).
* Magnitude edge of RSVLD_F16Q8: normalised activations beyond the e4m3 ranges of the cross terms (|x| > 64, > 112) against the
  host model of the saturating writer (include/rsvld_hip.h, RSVLD_HQ8_SX_*) and against plain fp64.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FOUR = ("attn", "attn_out", "ff", "qkv")      # the shipped composition's transformer groups


def _policies():
    from rsvld_amd import ops
    P = ops.SplitPolicy
    return {
        "UNET_POLICY": ops.UNET_POLICY,
        "f16 conv1": P(f16_inputs=FOUR + ("conv1",)),
        "f16 conv2": P(f16_inputs=FOUR + ("conv2",)),
        "f16 conv1+conv2": P(f16_inputs=FOUR + ("conv1", "conv2")),
        "q8 none": P(q8_convs=()),
        "q8 conv1": P(q8_convs=("conv1",)),
        "q8 conv2": P(q8_convs=("conv2",)),
        "ALL_SPLIT": ops.ALL_SPLIT,
        "fp32 family": None,
    }


def _route(pol, group, eligible):
    """The kernel family policy ``pol`` names for the convolution behind norm group ``group``."""
    if pol is None:
        return "f32"
    if group in pol.f16_inputs:
        return "w2"
    if group in pol.q8_convs and eligible:
        return "q8"
    return "split"


def _kind(name):
    """Kernel family of a convolution launch name (ops.LaunchProfiler record, ``profile_detail`` suffix stripped); None: not a convolution."""
    base = name.split(" [")[0]
    if base.startswith("conv_f32"):
        return "f32"
    if not (base.startswith("conv_") or base.startswith("gemm_")):
        return None
    if base == "conv_halo_128_q8":
        return "q8"
    if base.endswith("_w2"):
        return "w2"
    if base.endswith("_split"):
        return "split"
    return "other"


# ---------------------------------------------------------------------------------------------------------------------------------
# ResBlock route matrix
RES_CASES = {
    # name: (B, H, W, C_in, C_out, concat split of the input, conv1 / conv2 q8-eligible at the default split_halo_min_wgs = 64)
    "320->640 1x1 skip": (2, 64, 64, 320, 640, None, True),          # 160 workgroups
    "decoder 1280+640->640": (2, 32, 64, 1920, 640, (1280, 640), True),   # 80 workgroups; the input a materialised concat (concat_c)
    "128->64": (2, 32, 64, 128, 64, None, False),                    # Cout = 64: below eligibility, three MFMAs under q8_convs
}


def _resblock(C_in, C_out, seed):
    from rsvld_amd.hipnn import HipNet
    from rsvld_amd.sgm.modules.diffusionmodules.openaimodel import ResBlock

    class Net(HipNet):
        def __init__(self):
            super().__init__()
            self.blk = ResBlock(C_in, 1280, 0.0, out_channels=C_out)

    torch.manual_seed(seed)
    net = Net()
    blk = net.blk
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for gn in (blk.in_layers[0], blk.out_layers[0]):
            gn.weight.copy_(1 + 0.2 * torch.randn(gn.weight.shape, generator=g))
            gn.bias.copy_(0.2 * torch.randn(gn.bias.shape, generator=g))
        conv2 = blk.out_layers[3]                   # zero_module'd in the model: non-zero here, so conv2 matters
        conv2.weight.copy_(torch.randn(conv2.weight.shape, generator=g) / math.sqrt(9 * C_out))
        conv2.bias.copy_(0.1 * torch.randn(conv2.bias.shape, generator=g))
    ref = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    return net, ref


def _resblock_fp64(ref, x, emb, has_skip):
    """openaimodel.ResBlock in float64 (NCHW): GN + SiLU, conv1 + Linear(SiLU(emb)), GN + SiLU, conv2 + skip."""
    p = lambda k: ref["blk." + k]
    h = F.silu(F.group_norm(x, 32, p("in_layers.0.weight"), p("in_layers.0.bias"), 1e-5))
    h = F.conv2d(h, p("in_layers.2.weight"), p("in_layers.2.bias"), padding=1)
    h = h + F.linear(F.silu(emb), p("emb_layers.1.weight"), p("emb_layers.1.bias"))[:, :, None, None]
    h = F.silu(F.group_norm(h, 32, p("out_layers.0.weight"), p("out_layers.0.bias"), 1e-5))
    h = F.conv2d(h, p("out_layers.3.weight"), p("out_layers.3.bias"), padding=1)
    skip = F.conv2d(x, p("skip_connection.weight"), p("skip_connection.bias")) if has_skip else x
    return h + skip


@pytest.mark.parametrize("case", list(RES_CASES))
def test_resblock_policy_routes(cuda, case):
    """Bounds, relative to the block output's range, are two layers in series of the per-layer tests' (4e-5 for q8 / split, 2e-3 for an
    fp16 input: test_gpu_split.py): 8e-5 and 4e-3; the fp32 family 1e-5.  Measured (MI355X, the three blocks): q8 / split 5.0-9.0e-6,
    one or both conv inputs in fp16 0.87-1.7e-4, fp32 family 0.6-2.3e-6."""
    from rsvld_amd import ops
    B, H, W, C_in, C_out, cat, eligible = RES_CASES[case]
    net, ref = _resblock(C_in, C_out, seed=C_in + C_out)
    net = net.to(cuda).eval()
    net.compute_dtype = torch.float32
    g = torch.Generator().manual_seed(H + C_in)
    parts = [torch.randn(B, c, H, W, generator=g) * s + m for c, s, m in zip(cat or (C_in,), (1.7, 0.8), (0.3, -0.2))]
    x = torch.cat(parts, 1)
    emb = torch.randn(B, 1280, generator=g)
    want = _resblock_fp64(ref, x.double(), emb.double(), C_in != C_out).permute(0, 2, 3, 1)
    rng = float(want.abs().max())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(cuda)
    xd = ops.concat_c(*[nhwc(t) for t in parts]) if cat else nhwc(x)
    embd = emb.to(cuda)
    keys = {"conv1": f" [{B}x{H}x{W} {C_in}+0->{C_out} k3 s1]", "conv2": f" [{B}x{H}x{W} {C_out}+0->{C_out} k3 s1]"}
    assert keys["conv1"] != keys["conv2"]

    def run(pol, prof=None):
        with ops.f32_split(pol), ops.tuning(profiler=prof, profile_detail=prof is not None), torch.no_grad():
            return net.blk.run(net, xd, net.emb_rows(embd)).clone()

    failures, rows = [], []
    for name, pol in _policies().items():
        prof = ops.LaunchProfiler()
        got = run(pol, prof)
        again = run(pol)
        names = [r[0] for r in prof.records]
        convs = [(n, _kind(n)) for n in names if _kind(n) is not None]
        want_route = {grp: _route(pol, grp, eligible) for grp in ("conv1", "conv2")}
        if pol is None:
            n_f32 = 3 if C_in != C_out else 2
            if [k for _, k in convs] != ["f32"] * n_f32:
                failures.append(f"{name}: convolutions {convs}, expected {n_f32} x conv_f32")
        else:
            for grp, key in keys.items():
                seen = [k for n, k in convs if n.endswith(key)]
                if seen != [want_route[grp]]:
                    failures.append(f"{name}: {grp} ({key.strip()}) ran {seen}, the policy names {want_route[grp]}")
            others = [(n, k) for n, k in convs if not any(n.endswith(key) for key in keys.values())]
            if any(" k3 " in n for n, _ in others) or any(k != "split" for _, k in others):
                failures.append(f"{name}: unexpected convolutions {others}")   # only the 1x1 skip, in three MFMAs
            n_q8 = list(want_route.values()).count("q8")
            if names.count("groupnorm_apply_q8") != n_q8:
                failures.append(f"{name}: {names.count('groupnorm_apply_q8')} x groupnorm_apply_q8 for {n_q8} q8 convolutions")
        f16 = pol is not None and bool({"conv1", "conv2"} & pol.f16_inputs)
        bound = 4e-3 if f16 else 1e-5 if pol is None else 8e-5
        e = float((got.double().cpu() - want).abs().max()) / rng
        rows.append(f"   {name:18s} conv1 {want_route['conv1']:5s} conv2 {want_route['conv2']:5s} max|d| / range = {e:.2e} (bound {bound:.0e})")
        if not e <= bound:
            failures.append(f"{name}: {e:.3e} of the range {rng:.2f} > {bound}")
        if not torch.equal(got, again):
            failures.append(f"{name}: two runs differ")
    print(f"ResBlock {case}:\n" + "\n".join(rows))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# Call-site census in whole networks
def _census_nets(cuda):
    """The ControlNet + UNet of Stage 2 at SDXL channel widths (320 / 640 / 1280) and the reduced depth of the goldens
    (tests/golden/s2_common.py), initialised on the device (the routes do not depend on the values)."""
    import copy
    import os
    import sys
    import yaml
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import s2_common as S
    from rsvld_amd.sgm.util import instantiate_from_config
    cfg = yaml.safe_load(open(S.YAML))["model"]["params"]
    nets = {}
    torch.manual_seed(11)
    for name, key in (("ControlNet", "control_stage_config"), ("UNet", "network_config")):
        c = copy.deepcopy(cfg[key])
        c["params"].update(copy.deepcopy(S.SMALL))
        with torch.device(cuda):
            net = instantiate_from_config(c)
        net.compute_dtype = torch.float32
        nets[name] = net.eval()
    return nets, S.SMALL


def test_q8_call_site_census(cuda, monkeypatch):
    """At latent 64 and batch 2 (the CFG pair) the 320-channel ResBlocks are q8-eligible and the 640 / 1280-channel ones are not
    (40 workgroups < split_halo_min_wgs): the count is neither all nor none of them.  Measured: ControlNet 4 of 16 convolutions,
    UNet 10 of 34."""
    from rsvld_amd import _lib as L, ops
    from rsvld_amd.sgm.modules.diffusionmodules.openaimodel import ResBlock
    nets, small = _census_nets(cuda)
    B, lat = 2, 64
    g = torch.Generator().manual_seed(5)
    xt = ops.nchw_to_nhwc(torch.randn(B, 4, lat, lat, generator=g).to(cuda), torch.float32)
    hint = ops.nchw_to_nhwc(torch.randn(B, 4, lat, lat, generator=g).to(cuda), torch.float32)
    t = torch.tensor([500.0, 500.0], device=cuda)
    ctx = torch.randn(B, 77, small["context_dim"], generator=g).to(cuda)
    y = torch.randn(B, small["adm_in_channels"], generator=g).to(cuda)

    seen = []
    orig = ResBlock.run

    def census_run(self, rt, x, emb_rows):
        Bx, Hx, Wx, Cx = x.shape
        c1, c2 = self.in_layers[2], self.out_layers[3]
        ok = lambda conv, cin: bool(ops._q8_conv_eligible(Bx, Hx, Wx, cin, rt.pk(conv), 1, conv.padding[0], False, L.ACT_NONE, False))
        seen.append((id(self), ok(c1, Cx), ok(c2, self.out_channels)))
        return orig(self, rt, x, emb_rows)

    monkeypatch.setattr(ResBlock, "run", census_run)
    control = None
    for name in ("ControlNet", "UNet"):
        net = nets[name]
        blocks = [m for m in net.modules() if isinstance(m, ResBlock)]
        for pol, groups in ((ops.UNET_POLICY, (0, 1)), (ops.SplitPolicy(q8_convs=("conv1",)), (0,)), (ops.SplitPolicy(q8_convs=("conv2",)), (1,))):
            seen.clear()
            prof = ops.LaunchProfiler()
            with ops.f32_split(pol), ops.tuning(profiler=prof), torch.no_grad():
                if name == "ControlNet":
                    out = net(hint, t, xt, context=ctx, y=y)
                    control = out if pol is ops.UNET_POLICY else control
                else:
                    net(xt, timesteps=t, context=ctx, y=y, control=control)
            assert sorted(s[0] for s in seen) == sorted(id(m) for m in blocks), f"{name}: not every ResBlock of the module tree ran once"
            eligible = sum(s[1 + i] for s in seen for i in groups)
            names = [r[0] for r in prof.records]
            n_q8, n_apply = names.count("conv_halo_128_q8"), names.count("groupnorm_apply_q8")
            print(f"{name} {sorted(pol.q8_convs)}: {len(blocks)} ResBlocks, {eligible} eligible convolutions, {n_q8} q8 launches")
            assert n_q8 == eligible and n_apply == eligible, (name, pol, n_q8, n_apply, eligible)
            if pol is ops.UNET_POLICY:
                n_all = 2 * len(blocks)
                assert 0 < eligible < n_all, (name, eligible, n_all)


# ---------------------------------------------------------------------------------------------------------------------------------
# Magnitude edge of RSVLD_F16Q8
def _q8_parts(v, s_hi, s_lo):
    """host model of st_hq8 (include/rsvld_hip.h): (fp16 part, e4m3(v 2^s_hi) / 2^s_hi, e4m3((v - fp16 v) 2^s_lo) / 2^s_lo), the e4m3
    parts saturating at +-448 -- all fp64"""
    h = v.half().float()
    q = lambda t, s: (t * 2.0 ** s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double() / 2.0 ** s
    return h.double(), q(v, s_hi), q(v - h, s_lo)


def test_q8_saturation_range(cuda):
    """GroupNorm gamma 30-90 puts the normalised activations well past both e4m3 limits of the activation's cross terms (x_lo from
    |x| ~ 64, x_hi above 112).  (a) The q8 rows the GroupNorm apply pass writes are, bit for bit, the host model's saturating casts of
    the same fp32 tensor: no inf / NaN byte; (b) the convolution agrees with the host model's arithmetic at 5e-6 of the range (the bound
    of test_gpu_split.py::test_conv3x3_q8_cross_terms); (c) its distance from plain fp64 is no larger than the fp16-input form's
    (weight pairs) of the same layer.  Measured (MI355X, |x| up to 351): (b) 7.6e-7, (c) q8 1.07e-4 vs fp16 input 2.2e-4 of the range."""
    from rsvld_amd import ops
    B, H, W, C, Co = 2, 16, 48, 128, 128
    g = torch.Generator().manual_seed(64)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
    w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(Co, generator=g) * 0.1
    gamma = 30 + 60 * torch.rand(C, generator=g)
    beta = 2 * torch.randn(C, generator=g)
    pc = ops.pack_conv(w, b, torch.float32, cuda)
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    norm = (gamma.to(cuda), beta.to(cuda), 32, 1e-5, True)
    with ops.f32_split(ops.UNET_POLICY), ops.tuning(split_halo_min_wgs=0, profiler=(prof := ops.LaunchProfiler())):
        got = ops.conv2d(xd, pc, norm=norm, stats=True, norm_group="conv1")
        ab = ops._gn_scale_shift_f32(xd, None, norm[0], norm[1], 32, 1e-5)
        xn = ops._gn_apply_split(xd, None, ab, True, planes=False)                  # the fp32 tensor the q8 apply pass quantises
        rows = ops._gn_apply_split(xd, None, ab, True, planes=True, q8=True).t.cpu()
    assert {"conv_halo_128_q8", "groupnorm_apply_q8"} <= set(prof.summary())
    with ops.f32_split(ops.SplitPolicy(f16_inputs=FOUR + ("conv1",))), ops.tuning(split_halo_min_wgs=0, profiler=(prof16 := ops.LaunchProfiler())):
        f16 = ops.conv2d(xd, pc, norm=norm, stats=True, norm_group="conv1")
    assert any(n.endswith("_w2") for n in prof16.summary()) and "conv_halo_128_q8" not in prof16.summary()
    xn = xn.cpu()
    a = xn.abs()
    n_lo, n_hi = int(((a > 64) & (a <= 112)).sum()), int((a > 112).sum())
    print(f"normalised activations: max {float(a.max()):.1f}; {n_lo} in (64, 112], {n_hi} above 112 of {a.numel()}")
    assert n_lo > 1000 and n_hi > 1000
    # (a) the row format, bit for bit
    h16 = rows[..., 0, :].float()
    blocks = rows[..., 1, :].contiguous().view(torch.uint8).view(B, H, W, C // 32, 4, 16)
    p0 = torch.cat([blocks[..., 0, :], blocks[..., 2, :]], -1).reshape(B, H, W, C).view(torch.float8_e4m3fn).float()
    p1 = torch.cat([blocks[..., 1, :], blocks[..., 3, :]], -1).reshape(B, H, W, C).view(torch.float8_e4m3fn).float()
    hh = xn.half().float()
    want0 = ((xn - hh) * 2.0 ** 14).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    want1 = (xn * 4.0).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    assert torch.isfinite(p0).all() and torch.isfinite(p1).all() and torch.isfinite(got).all()
    assert torch.equal(h16, hh), int((h16 != hh).sum())
    assert torch.equal(p0, want0), int((p0 != want0).sum())
    assert torch.equal(p1, want1), int((p1 != want1).sum())
    assert float(p0.abs().max()) == 448.0 and float(p1.abs().max()) == 448.0       # both parts did saturate
    # (b) the arithmetic of the saturating model
    wp = pc.w.cpu().view(Co, 3, 3, C).permute(0, 3, 1, 2)
    xh, xq, xlq = _q8_parts(xn.permute(0, 3, 1, 2), 2, 14)
    wh, wq, wlq = _q8_parts(wp, 6, 18)
    conv = lambda u, ww: F.conv2d(u, ww, None, padding=1)
    model = conv(xh, wh) + conv(xlq, wq) + conv(xq, wlq) + b.double().view(1, -1, 1, 1)
    got_c = got.double().cpu().permute(0, 3, 1, 2)
    rng = float(model.abs().max())
    e_model = float((got_c - model).abs().max())
    # (c) plain fp64 of the layer, and the fp16-input form
    ye = F.conv2d(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5)), w.double(), b.double(), padding=1)
    e_q8 = float((got_c - ye).abs().max())
    e_f16 = float((f16.double().cpu().permute(0, 3, 1, 2) - ye).abs().max())
    print(f"q8 at |x| up to {float(a.max()):.0f}: vs the saturating model {e_model / rng:.2e}, vs fp64 {e_q8 / rng:.2e} "
          f"(fp16-input form {e_f16 / rng:.2e}) of the range {rng:.1f}")
    assert e_model <= 5e-6 * rng
    assert e_q8 <= e_f16
