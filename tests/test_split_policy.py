"""Host tests of the split precision's policy layer (rsvld_amd.ops.SplitPolicy) and of the q8 eligibility that routes a ResBlock
convolution to RSVLD_F16Q8 -- no GPU: the policy is plain Python, and rsvld_conv3x3_halo_supported is host code of the library.

* Every combination of the constructor's arguments raises ValueError exactly when one of the rules its docstring states is broken (the
  rules are restated here, not derived from the constructor), and every policy that builds is consistent.
* Every policy the measurement tools and bench.py's policy options build is constructible (a policy that raises there ends a run).
* ``ops._q8_conv_eligible`` (Python) never accepts a layer that rsvld_conv3x3_halo_supported (C) refuses -- ``_conv2d_q8`` would raise in
  the middle of a network -- and accepts every layer C accepts once the Python-only conditions (fp32 weights, the halo route, the
  workgroup threshold) hold -- otherwise the layer silently runs as three bf16 MFMAs.
"""
import ctypes
import itertools
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRANSFORMER = ("attn", "attn_out", "ff", "qkv")          # the shipped composition's transformer groups
WEIGHT_INPUT = {"qkv": "qkv", "geglu": "ff", "attn_out": "attn_out", "ff_out": "ff"}   # weight group -> the input group it needs


def _subsets(xs):
    return [tuple(c) for r in range(len(xs) + 1) for c in itertools.combinations(xs, r)]


def _expected(impl, fi, fw, q8):
    """The documented rules, restated: -> (q8_convs, f16_weights) of the policy, or None where the constructor must raise ValueError."""
    fi = set(fi)
    if q8 is None:        # default: the ResBlock convolutions that f16_inputs does not round, in the shipped composition's product path
        q8 = tuple(g for g in ("conv1", "conv2") if g not in fi) if impl == "planes" and set(TRANSFORMER) <= fi else ()
    if set(q8) & fi:                                   # a convolution input is fp16 OR e4m3 cross terms
        return None
    if q8 and impl != "planes":                        # q8 exists in the product path only
        return None
    if fw is None:        # default: every transformer GEMM whose input is fp16
        fw = tuple(w for w, i in WEIGHT_INPUT.items() if i in fi and impl == "planes")
    if (fi - {"attn"}) and "attn" not in fi:           # fp16 layer inputs go with fp16 attention operands
        return None
    if fi and impl != "planes":                        # fp16 inputs exist in the product path only
        return None
    if any(WEIGHT_INPUT[w] not in fi for w in fw):     # a weight is rounded only where its layer's input is
        return None
    return frozenset(q8), frozenset(fw)


def test_constructor_sweep_raises_exactly_on_broken_rules():
    from rsvld_amd import ops
    P = ops.SplitPolicy
    built, n = [], 0
    for impl in ("planes", "f32"):
        for fi in _subsets(P.GROUPS):
            for fw in [None] + _subsets(P.WEIGHT_GROUPS):
                for q8 in (None, (), ("conv1",), ("conv2",), ("conv1", "conv2")):
                    n += 1
                    want = _expected(impl, fi, fw, q8)
                    args = dict(impl=impl, f16_inputs=fi, f16_weights=fw, q8_convs=q8)
                    if want is None:
                        with pytest.raises(ValueError):
                            P(**args)
                        continue
                    p = P(**args)
                    assert (p.q8_convs, p.f16_weights) == want, args
                    assert p.impl == impl and p.f16_inputs == frozenset(fi), args
                    assert not p.q8_convs & p.f16_inputs, args
                    assert all(WEIGHT_INPUT[w] in p.f16_inputs for w in p.f16_weights), args
                    assert p.q8_convs <= set(P.Q8_GROUPS) and p.f16_weights <= set(P.WEIGHT_GROUPS), args
                    d = p.describe()
                    again = P(impl=d["impl"], f16_inputs=d["f16_inputs"], f16_weights=d["f16_weights"], q8_convs=d["q8_convs"])
                    assert again == p and hash(again) == hash(p) and again.key() == p.key(), args
                    built.append(p)
    assert n == 2 * 2 ** 7 * (2 ** 4 + 1) * 5
    keys = {p.key() for p in built}
    # == and hash follow key(): equal keys collapse in a set, different keys never do
    assert len(set(built)) == len(keys)
    by_key = {}
    for p in built:
        q = by_key.setdefault(p.key(), p)
        assert q == p and hash(q) == hash(p)
    reps = list(by_key.values())
    assert all((a == b) == (a.key() == b.key()) for a, b in zip(reps, reps[1:] + reps[:1]))
    print(f"{n} combinations, {len(built)} build, {len(keys)} distinct policies")


def test_default_derivation_of_q8_convs():
    from rsvld_amd import ops
    P = ops.SplitPolicy
    # the shipped composition: unchanged, and with it the hipGraph key and bench.py's headline
    assert P() == ops.UNET_POLICY and ops.UNET_POLICY.q8_convs == {"conv1", "conv2"}
    assert ops.UNET_POLICY.key() == ("planes", ("attn", "attn_out", "ff", "qkv"), ("attn_out", "ff_out", "geglu", "qkv"), ("conv1", "conv2"))
    assert ops.ALL_SPLIT.q8_convs == frozenset() and ops.VAE_POLICY.q8_convs == frozenset()
    # a group that f16_inputs rounds to fp16 leaves the default's q8 set; the other one stays in it
    assert P(f16_inputs=TRANSFORMER + ("conv1",)).q8_convs == {"conv2"}
    assert P(f16_inputs=TRANSFORMER + ("conv2",)).q8_convs == {"conv1"}
    assert P(f16_inputs=TRANSFORMER + ("conv1", "conv2")).q8_convs == frozenset()
    assert P(f16_inputs=TRANSFORMER + ("proj",)).q8_convs == {"conv1", "conv2"}
    # not the shipped composition: no q8 unless asked for
    assert P(f16_inputs=("attn", "attn_out", "ff")).q8_convs == frozenset()
    assert P(f16_inputs=("attn",)).q8_convs == frozenset()
    assert P(impl="f32", f16_inputs=(), f16_weights=()).q8_convs == frozenset()
    assert P(f16_inputs=(), f16_weights=(), q8_convs=("conv2",)).q8_convs == {"conv2"}
    # an explicit overlap is still an error
    for g in ("conv1", "conv2"):
        with pytest.raises(ValueError, match="either rounded to fp16"):
            P(f16_inputs=TRANSFORMER + (g,), q8_convs=(g,))


def test_tolerance_check_modes_build():
    """tools/tolerance_check.py builds its whole table before ``--only`` selects from it: every entry must construct."""
    from rsvld_amd import ops
    from tools import tolerance_check
    modes = tolerance_check.modes()
    assert {"shipped", "split", "split_noconv", "split_conv", "split_conv2", "split_noq8", "split_full"} <= set(modes)
    for name, (s1, ae, df, pol, pol1) in modes.items():
        assert pol is None or isinstance(pol, ops.SplitPolicy), name
        assert pol1 is None or isinstance(pol1, ops.SplitPolicy), name
    assert modes["split_noconv"][3].q8_convs == frozenset()          # round 5's three-MFMA convolutions, as its name says
    assert modes["split_noq8"][3].q8_convs == frozenset()
    assert modes["split_conv"][3].q8_convs == frozenset()
    assert modes["split_conv2"][3].q8_convs == {"conv1"} and "conv2" in modes["split_conv2"][3].f16_inputs
    assert modes["split_full"][3] == ops.ALL_SPLIT


def _bench_policy(unet_f16_groups=None, unet_f16_weights=None, unet_q8_convs=None):
    """bench.py's ``--unet-f16-groups`` / ``--unet-f16-weights`` / ``--unet-q8-convs`` -> the policy, in the form of its call."""
    from rsvld_amd import ops
    gi = ops.UNET_POLICY.f16_inputs if unet_f16_groups is None else tuple(g for g in unet_f16_groups.split(",") if g)
    gw = None if unet_f16_weights is None else tuple(g for g in unet_f16_weights.split(",") if g)
    gq = None if unet_q8_convs is None else tuple(g for g in unet_q8_convs.split(",") if g)
    return ops.SplitPolicy(f16_inputs=tuple(gi), f16_weights=gw, q8_convs=gq)


def test_bench_policy_options_build():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "UNET_POLICY = ops.SplitPolicy(f16_inputs=tuple(gi), f16_weights=gw, q8_convs=gq)" in src, "bench.py's policy call changed"
    four = ",".join(TRANSFORMER)
    cases = [
        (dict(unet_f16_groups=four), {"conv1", "conv2"}),
        (dict(unet_f16_groups=four + ",conv1"), {"conv2"}),
        (dict(unet_f16_groups=four + ",conv2"), {"conv1"}),
        (dict(unet_f16_groups=four + ",conv1,conv2"), set()),
        (dict(unet_f16_groups=four + ",proj"), {"conv1", "conv2"}),
        (dict(unet_q8_convs=""), set()),
        (dict(unet_q8_convs="conv1"), {"conv1"}),
        (dict(unet_q8_convs="conv2"), {"conv2"}),
        (dict(unet_f16_weights=""), {"conv1", "conv2"}),
    ]
    for kw, q8 in cases:
        p = _bench_policy(**kw)
        assert p.q8_convs == q8, (kw, p)
        assert "conv1" not in p.q8_convs or "conv1" not in p.f16_inputs
    assert _bench_policy(unet_f16_weights="").f16_weights == frozenset()
    from rsvld_amd import ops
    assert _bench_policy(unet_f16_groups=four) == ops.UNET_POLICY


# ----------------------------------------------------------------------------- q8 eligibility: Python against the library's predicate
VARIANTS = {          # name -> (kernel size, keyword arguments of the layer)
    "3x3": (3, dict(pad=1)),
    "pad None": (3, dict(pad=None)),
    "pad 4-tuple": (3, dict(pad=(1, 1, 1, 1))),
    "upsample": (3, dict(pad=1, upsample=True)),
    "stride 2": (3, dict(pad=1, stride=2)),
    "pad 0": (3, dict(pad=0)),
    "GEGLU": (3, dict(pad=1, act="geglu")),
    "planes out": (3, dict(pad=1, out_planes=True)),
    "1x1": (1, dict(pad=0)),
}


def _workgroups(B, H, W, cout_p, plan_div):
    return -(-B // plan_div) * ((H + 7) // 8) * ((W + 31) // 32) * ((cout_p + 127) // 128)


def test_q8_eligibility_agrees_with_the_library():
    from rsvld_amd import _lib as L, ops
    lib = L.load()
    packs = {}
    n_py = n_c = n = 0
    for Cin, Cout, k, wdt in itertools.product((32, 64, 96, 128, 1920), (8, 64, 72, 128, 320), (3, 1), (torch.float32, torch.float16)):
        packs[Cin, Cout, k, wdt] = ops.pack_conv(torch.zeros(Cout, Cin, k, k), torch.zeros(Cout), wdt, "cpu")
    for (Cin, Cout, k, wdt), pc in packs.items():
        for H, W, B, plan_div, (vname, (vk, kw)) in itertools.product((3, 4, 5), (15, 16, 17, 33), (1, 3), (1, 2), VARIANTS.items()):
            if vk != k:
                continue
            kw = dict(kw)
            act = L.ACT_GEGLU if kw.pop("act", None) == "geglu" else L.ACT_NONE
            geo = dict(stride=kw.get("stride", 1), pad=kw["pad"], upsample=kw.get("upsample", False), act=act,
                       out_planes=kw.get("out_planes", False))
            wgs = _workgroups(B, H, W, pc.cout_p, plan_div)
            for min_wgs, use_halo in ((wgs, True), (wgs + 1, True), (0, False)):
                with ops.tuning(plan_div=plan_div, split_halo_min_wgs=min_wgs, use_halo=use_halo):
                    py = bool(ops._q8_conv_eligible(B, H, W, Cin, pc, geo["stride"], geo["pad"], geo["upsample"], act, geo["out_planes"]))
                    d = ops._q8_conv_desc(B, H, W, Cin, pc, **geo)
                    c = bool(lib.rsvld_conv3x3_halo_supported(ctypes.byref(d)))
                what = f"Cin {Cin} Cout {Cout} {vname} {B}x{H}x{W} w {wdt} plan_div {plan_div} min_wgs {min_wgs} (wgs {wgs}) halo {use_halo}"
                # Python must not accept what C refuses: _conv2d_q8 raises mid-network
                assert not py or c, "accepted by _q8_conv_eligible, refused by rsvld_conv3x3_halo_supported: " + what
                # C's acceptance + the Python-only conditions -> Python accepts (else the layer silently takes three bf16 MFMAs)
                py_only = wdt == torch.float32 and use_halo and wgs >= min_wgs
                assert py == (c and py_only), "refused by _q8_conv_eligible, accepted by rsvld_conv3x3_halo_supported: " + what
                n += 1
                n_py += py
                n_c += c
    print(f"{n} layer / context combinations: {n_py} eligible, {n_c} accepted by the library")
    assert n_py > 50 and n_c > n_py      # the sweep reaches both sides of every clause
