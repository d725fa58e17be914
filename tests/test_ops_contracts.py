"""Operand contracts of the public wrappers in ``rsvld_amd.ops`` (CPU and meta tensors, no GPU).

Every wrapper checks each operand it hands to a kernel -- dtype, the layout the kernel reads, shape agreement with the other
operands -- before it allocates, launches or asks for the GPU.  The table below holds one well-formed call per wrapper; for every
tensor operand of it a strided view, the wrong dtype and a wrong shape must raise ``RsvldOperandError`` (not the GPU-only error),
and the well-formed call itself must reach the GPU-only error.  ``test_table_covers_every_wrapper`` keeps the table complete."""
import inspect

import pytest
import torch

from rsvld_amd import _lib as L, ops

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def T(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype)


def _pc(cin, cout, k=1, dtype=F16, bias=True):
    return ops.pack_conv(torch.zeros(cout, cin, k, k), torch.zeros(cout) if bias else None, dtype, "cpu")


# name -> (wrapper, builder of the well-formed arguments (positional list, keyword dict), {operand: (wrong dtype, wrong shape)})
# Operands are addressed as an int (positional index) or a str (keyword).  Wrong shapes disagree with the other operands.
CASES = {
    "to_planes": (ops.to_planes, lambda: ([T(2, 3, 16)], {}), {0: (F16, (2, 3, 12))}),
    "to_q8rows": (ops.to_q8rows, lambda: ([T(2, 3, 64)], {}), {0: (F16, (2, 3, 48))}),
    "conv2d_f16": (ops.conv2d, lambda: ([T(1, 4, 6, 16, dtype=F16), _pc(24, 16, 3)],
                                        {"x2": T(1, 4, 6, 8, dtype=F16), "rowvec": T(1, 16), "residual": T(1, 4, 6, 16, dtype=F16)}),
                   {0: (F32, (1, 4, 6, 24)), "x2": (BF16, (1, 4, 5, 8)), "rowvec": (F16, (2, 16)), "residual": (F32, (1, 4, 6, 8))}),
    "conv2d_out_f32": (ops.conv2d, lambda: ([T(1, 4, 6, 16, dtype=BF16), _pc(16, 16, 1, BF16)], {"pad": 0, "out_f32": True,
                                                                                               "residual": T(1, 4, 6, 16)}),
                       {"residual": (BF16, (1, 4, 6, 24))}),
    "conv2d_f32": (ops.conv2d, lambda: ([T(1, 4, 6, 16), _pc(16, 8, 3, F32)], {"residual": T(1, 4, 6, 8),
                                                                                "norm": (T(16), T(16), 4, 1e-5, True)}),
                   {0: (torch.float64, (1, 4, 6, 8)), "residual": (F16, (1, 4, 4, 8))}),
    "conv2d_planes": (ops.conv2d, lambda: ([ops.Planes(T(1, 4, 6, 2, 16, dtype=BF16)), _pc(16, 8, 3, F32)], {"residual": T(1, 4, 6, 8)}),
                      {"residual": (F16, (1, 4, 6, 16))}),
    "linear": (ops.linear, lambda: ([T(2, 5, 16, dtype=F16), _pc(16, 32)], {"residual": T(2, 5, 32, dtype=F16)}),
               {0: (torch.float64, (2, 5, 24)), "residual": (F32, (2, 4, 32))}),
    "group_norm": (ops.group_norm, lambda: ([T(1, 4, 4, 32, dtype=F16), T(48), T(48), 8, 1e-5],
                                            {"x2": T(1, 4, 4, 16, dtype=F16), "mod_scale1p": T(1, 4, 4, 96, dtype=F16)[..., :48],
                                             "mod_shift": T(1, 4, 4, 96, dtype=F16)[..., 48:]}),
                   {0: (torch.float64, (1, 4, 4, 40)), 1: (F16, (32,)), 2: (F16, (56,)), "x2": (BF16, (1, 4, 2, 16)),
                    "mod_scale1p": (F32, (1, 4, 4, 40)), "mod_shift": (BF16, (1, 2, 4, 48))}),
    "group_norm_f32": (ops.group_norm, lambda: ([T(1, 4, 4, 32), T(32), T(32), 8, 1e-5], {}),
                       {1: (F16, (40,)), 2: (BF16, (16,))}),
    "group_norm_stats": (ops.group_norm_stats, lambda: ([T(2, 4, 4, 32, dtype=BF16), 8], {"x2": T(2, 4, 4, 8, dtype=BF16)}),
                         {0: (torch.int32, (2, 4, 4)), "x2": (F16, (1, 4, 4, 8))}),
    "group_norm_apply": (ops.group_norm_apply, lambda: ([T(2, 4, 4, 32, dtype=F16), T(2, 8, 2), T(40), T(40), 8, 1e-5],
                                                        {"x2": T(2, 4, 4, 8, dtype=F16)}),
                         {0: (torch.float64, (2, 4, 4, 24)), 1: (F16, (2, 4, 2)), 2: (F16, (32,)), 3: (BF16, (48,)),
                          "x2": (F32, (2, 4, 3, 8))}),
    "layer_norm": (ops.layer_norm, lambda: ([T(3, 7, 64, dtype=F16), T(64), T(64)], {}),
                   {0: (torch.float64, (3, 7)), 1: (F16, (72,)), 2: (BF16, (56,))}),
    "attention": (ops.attention, lambda: ([T(2, 5, 128, dtype=F16), T(2, 7, 128, dtype=F16), T(2, 7, 128, dtype=F16), 2], {}),
                  {0: (torch.float64, (2, 5, 127)), 1: (BF16, (2, 7, 64)), 2: (BF16, (2, 6, 128))}),
    "attention_f32": (ops.attention, lambda: ([T(1, 5, 64), T(1, 6, 64), T(1, 6, 64), 1], {}),
                      {1: (F16, (2, 6, 64)), 2: (BF16, (1, 6, 72))}),
    "attention_planes": (ops.attention, lambda: ([ops.Planes(T(1, 5, 2, 128, dtype=BF16)), T(1, 6, 128), T(1, 6, 128), 2], {}),
                         {1: (BF16, (1, 6, 64)), 2: (torch.float64, (1, 7, 128))}),
    "gemv": (ops.gemv, lambda: ([T(32, 64, dtype=F16), T(64, dtype=F16)], {"bias": T(32, dtype=F16)}),
             {0: (F32, (32,)), 1: (BF16, (48,)), "bias": (F32, (16,))}),
    "gemv_fused": (ops.gemv_fused, lambda: ([T(32, 64, dtype=BF16), T(128, dtype=BF16), T(32, dtype=BF16)],
                                            {"norm": None, "residual": T(32, dtype=BF16), "glu": True}),
                   {0: (F16, (32,)), 1: (F16, (64,)), 2: (F32, (31,)), "residual": (F32, (64,))}),
    "gemv_fused_norm": (ops.gemv_fused, lambda: ([T(32, 64, dtype=F16), T(64, dtype=F16)], {"norm": (T(64, dtype=F16), 1e-6)}),
                        {}),
    "llama_decode_attention": (ops.llama_decode_attention,
                               lambda: ([T(8 * 128, dtype=F16), T(128, dtype=F16), T(128, dtype=F16), torch.zeros((), dtype=torch.int64),
                                         T(2, 16, 128, dtype=F16), T(2, 16, 128, dtype=F16), 4, 2, 0.1], {"ws": T(4096)}),
                               {0: (BF16, (7 * 128,)), 1: (F32, (64,)), 2: (BF16, (127,)), 3: (torch.int32, (2,)),
                                4: (BF16, (3, 16, 128)), 5: (F32, (2, 8, 128)), "ws": (F16, (64, 64))}),
    "linear_small": (ops.linear_small, lambda: ([T(3, 40), T(6, 40), T(6)], {}),
                     {0: (F16, (3, 41)), 1: (F16, (6, 32)), 2: (torch.float64, (5,))}),
    "sinusoidal": (ops.sinusoidal, lambda: ([T(4), 16, 0], {}), {0: (torch.bool, None)}),
    "nchw_to_nhwc": (ops.nchw_to_nhwc, lambda: ([T(1, 3, 4, 5), F16], {"out": T(1, 4, 5, 8, dtype=F16), "c_off": 2}),
                     {0: (torch.int32, (1, 3, 4)), "out": (torch.float64, (1, 4, 5, 4))}),
    "nhwc_to_nchw": (ops.nhwc_to_nchw, lambda: ([T(1, 4, 5, 8, dtype=BF16)], {"channels": 3, "c_off": 4}),
                     {0: (torch.float64, (1, 4, 5, 4))}),
    "axpby": (ops.axpby, lambda: ([T(2, 4, 16, dtype=BF16), T(2, 4, 16, dtype=BF16), 0.5, 0.5], {}),
              {0: (torch.float64, None), 1: (F16, (2, 4, 8))}),
    "geglu": (ops.geglu, lambda: ([T(3, 5, 32, dtype=F16)], {}), {0: (F32, (3, 5, 31))}),
    "ddpm_step": (ops.ddpm_step, lambda: ([T(1, 3, 4, 5), T(1, 4, 5, 8), T(1, 3, 4, 5), 1.0, 0.1, 0.5, 0.5, 0.1], {}),
                  {0: (F16, (1, 3, 4)), 1: (F16, (1, 4, 5, 2)), 2: (F16, (1, 3, 5, 4))}),
    "denoiser_out": (ops.denoiser_out, lambda: ([T(2, 4, 5, 8), T(2, 4, 4, 5), 0.5, 1.0], {}),
                     {0: (F16, (2, 4, 5, 3)), 1: (F16, (2, 4, 5, 4))}),
    "lerp_f32": (ops.lerp_f32, lambda: ([T(2, 4, 8, 8), T(2, 4, 8, 8), 7.5], {}), {0: (F16, None), 1: (F16, (2, 4, 8, 4))}),
    "axpy_f32": (ops.axpy_f32, lambda: ([T(2, 4, 8, 8), T(2, 4, 8, 8), 0.3], {}), {0: (F16, (2, 4, 8, 7)), 1: (F16, None)}),
    "euler_step": (ops.euler_step, lambda: ([T(1, 4, 8, 8), T(1, 4, 8, 8), T(1, 4, 8, 8), 0.1, 2.0, -0.5], {}),
                   {0: (F16, None), 1: (BF16, (1, 4, 8, 16)), 2: (torch.float64, (4, 8, 8))}),
    "tile_blend_accumulate": (ops.tile_blend_accumulate, lambda: ([T(1, 4, 8, 8), T(1, 4, 8, 8), T(1, 4, 4, 6), T(4, 6), 2, 1], {}),
                              {0: (F16, (1, 4, 8, 6)), 1: (F16, (1, 4, 8, 9)), 2: (F16, (1, 4, 4, 8)), 3: (F16, (6, 4))}),
    "tile_blend_finish": (ops.tile_blend_finish, lambda: ([T(1, 4, 8, 8), T(1, 4, 8, 8)], {}),
                          {0: (F16, None), 1: (F16, (1, 4, 8, 16))}),
    "absdiff_sums": (ops.absdiff_sums, lambda: ([T(2, 4, 4, 8, dtype=F16), T(2, 4, 4, 8, dtype=F16)], {}),
                     {0: (torch.float64, None), 1: (BF16, (1, 4, 4, 8))}),
    "gaussian_sample": (ops.gaussian_sample, lambda: ([T(1, 4, 5, 8, dtype=BF16), 4, T(1, 4, 4, 5), 0.18], {}),
                        {0: (torch.float64, (1, 4, 5, 6)), 2: (F16, (1, 4, 5, 4))}),
    "wavelet_blur": (ops.wavelet_blur, lambda: ([T(1, 3, 8, 8), 2], {"high_accum": T(1, 3, 8, 8)}),
                     {0: (F16, (3, 8, 8)), "high_accum": (F16, (1, 3, 4, 4))}),
    "add_f32": (ops.add_f32, lambda: ([T(2, 3, 4, 4), T(2, 3, 4, 4)], {}), {0: (F16, None), 1: (F16, (2, 3, 4))}),
    "adain": (ops.adain, lambda: ([T(1, 3, 8, 8), T(1, 3, 8, 8)], {}), {0: (F16, (3, 8, 8)), 1: (F16, (1, 3, 4, 4))}),
    "concat_c": (ops.concat_c, lambda: ([T(2, 3, 16, dtype=F16), T(2, 3, 8, dtype=F16)], {}),
                 {0: (torch.float64, None), 1: (BF16, (2, 4, 8))}),
    "concat_c_f32": (ops.concat_c, lambda: ([T(2, 3, 8), T(2, 3, 16)], {}), {1: (F16, (3, 3, 16))}),
}

# public callables of ops.py that launch nothing on their own operands, with the reason
ALLOWED = {
    "pad8": "integer arithmetic",
    "context": "returns the launch context",
    "tuning": "context manager over the launch context",
    "set_defaults": "changes the launch context",
    "plan_units": "context manager over the launch context",
    "f32_split": "context manager over the launch context",
    "precision_token": "returns a hashable key",
    "f16_group": "policy query",
    "q8_group": "policy query",
    "set_profiler": "changes the launch context",
    "pack_conv": "host-side torch re-layout of a weight; its result is checked by conv2d / linear",
    "as_f32": "delegates to Planes.f32, which copies to contiguous planes first",
    "maybe_planes": "passes every operand through except a contiguous fp32 tensor with C % 8 == 0, which goes to to_planes",
    "LaunchContext": "class: launch settings", "SplitPolicy": "class: precision policy", "LaunchProfiler": "class: HIP-event timing",
    "PackedConv": "class: weight container, checked by conv2d / linear", "Planes": "class: split-form container",
    "Q8Rows": "class: e4m3 row container, read only by the q8 convolution",
}


def _call(case, device, mutate=None):
    fn, build, _ = CASES[case]
    args, kw = build()

    def move(v):
        if isinstance(v, torch.Tensor):
            return v.to(device)
        if isinstance(v, ops.Planes):
            return ops.Planes(v.t.to(device))
        if isinstance(v, tuple):
            return tuple(move(e) for e in v)
        return v
    args, kw = [move(a) for a in args], {k: move(v) for k, v in kw.items()}
    if mutate is not None:
        key, new = mutate
        if isinstance(key, int):
            args[key] = new(args[key])
        else:
            kw[key] = new(kw[key])
    return fn(*args, **kw)


def _strided(t):
    """The same shape and dtype as a view with inner stride 2 inside a larger contiguous buffer."""
    base = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    return base[..., ::2]


# operands without a layout of their own to break: copied by the wrapper on purpose, or a 0-d scalar
NO_VIEW = {("sinusoidal", 0), ("nchw_to_nhwc", 0), ("llama_decode_attention", 3)}
# wrappers whose shape checks sit in the wrapper they delegate to
DELEGATES = {"linear": "conv2d"}


def _rows():
    out = []
    for case, (_, _, bad) in CASES.items():
        for key, (wrong_dt, wrong_shape) in bad.items():
            if (case, key) not in NO_VIEW:
                out.append((case, key, "view"))
            out.append((case, key, "dtype"))
            if wrong_shape is not None:
                out.append((case, key, "shape"))
    return out


@pytest.fixture(params=["cpu", "meta"])
def device(request):
    return torch.device(request.param)


@pytest.mark.parametrize("case", sorted(CASES))
def test_well_formed_call_reaches_the_gpu_check(case, device):
    with pytest.raises(L.RsvldError) as e:
        _call(case, device)
    assert not isinstance(e.value, L.RsvldOperandError), str(e.value)
    assert "GPU only" in str(e.value)


@pytest.mark.parametrize("case,key,kind", _rows(), ids=lambda v: str(v))
def test_bad_operand_is_rejected_before_launch(case, key, kind, device):
    wrong_dt, wrong_shape = CASES[case][2][key]
    if kind == "view":
        new = _strided
    elif kind == "dtype":
        new = lambda t: torch.zeros(t.shape, dtype=wrong_dt, device=t.device)
    else:
        new = lambda t: torch.zeros(wrong_shape, dtype=t.dtype, device=t.device)
    with pytest.raises(L.RsvldOperandError) as e:
        _call(case, device, (key, new))
    fn = CASES[case][0].__name__
    assert e.value.args[0].split(":")[0] in (fn, DELEGATES.get(fn)), str(e.value)


def test_table_covers_every_wrapper():
    public = {n for n, v in vars(ops).items() if not n.startswith("_") and (inspect.isfunction(v) or inspect.isclass(v))
              and getattr(v, "__module__", None) == ops.__name__}
    covered = {fn.__name__ for fn, _, _ in CASES.values()}
    missing = public - covered - set(ALLOWED)
    assert not missing, f"public wrappers without contract rows: {sorted(missing)}"
    assert not (set(ALLOWED) - public), f"stale allow-list entries: {sorted(set(ALLOWED) - public)}"
    for case, (fn, _, bad) in CASES.items():
        assert bad or case.endswith("_norm"), case


def test_operand_error_is_an_rsvld_error_and_a_value_error():
    assert issubclass(L.RsvldOperandError, L.RsvldError) and issubclass(L.RsvldOperandError, ValueError)


def test_supported_views_pass_the_contract(device):
    """Views the wrappers read in place -- q | k | v token-stride slices of one fused tensor, channel-slice modulation -- are not
    operand errors (they reach the GPU-only check)."""
    qkv = torch.zeros(2, 9, 3 * 128, dtype=F16, device=device)
    with pytest.raises(L.RsvldError) as e:
        ops.attention(qkv[..., :128], qkv[..., 128:256], qkv[..., 256:], heads=2)
    assert not isinstance(e.value, L.RsvldOperandError), str(e.value)
    # a misaligned token-stride view is not one of them
    with pytest.raises(L.RsvldOperandError):
        ops.attention(qkv[..., 4:132], qkv[..., 128:256], qkv[..., 256:], heads=2)
