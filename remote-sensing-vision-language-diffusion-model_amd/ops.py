"""Tensor-level wrappers over the C ABI (include/rsvld_hip.h).

torch is used here only for device memory (allocation through its caching allocator) and for the
current HIP stream; every computation is a kernel of librsvld_hip.so.  Activations are NHWC
16-bit tensors ``[B, H, W, C]`` with ``C % 8 == 0``; tokens ``[B, N, C]`` are the same thing with
``H = 1``.  Every function raises if the tensor is not on a GPU: there is no CPU path.

fp32 activations select the fp32-operand family (csrc/f32.hip): ``conv2d`` /
``linear``, ``group_norm*``, ``layer_norm``, ``attention``, ``concat_c``, ``axpby``, ``absdiff_sums`` and ``nchw_to_nhwc``
dispatch on the tensor's dtype (the VAE under ``ae_dtype: fp32``, the UNet / ControlNet under ``diffusion_dtype: fp32``).
"""
import contextlib
import ctypes as C
import contextvars
import math

import torch

from . import _lib as L

_DT = {torch.float16: L.F16, torch.bfloat16: L.BF16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.RsvldError("rsvld_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise L.RsvldError(f"16-bit activation expected, got {t.dtype}")


def pad8(c):
    return (c + 7) // 8 * 8


# ----------------------------------------------------------------------------- operand contracts
# The C ABI takes raw pointers and sizes read off ONE operand, so a wrong operand would give plausible numbers or an access past
# another operand's allocation.  Every public wrapper therefore checks each operand -- dtype, the layout the kernel reads, shape
# agreement -- before it allocates, launches or asks for the GPU (checked before ``_need_gpu``: a CPU or meta tensor exercises the
# contract, tests/test_ops_contracts.py) and raises ``RsvldOperandError`` naming the wrapper and the operand.
_HALF = (torch.float16, torch.bfloat16)
_ACT = (torch.float16, torch.bfloat16, torch.float32)


def _bad(fn, name, what):
    raise L.RsvldOperandError(f"{fn}: operand '{name}' {what}")


def _arg(fn, name, t, dtype=None, shape=None, numel=None, layout="contiguous", optional=False):
    """Contract of operand ``name`` of wrapper ``fn``.  ``dtype``: one dtype or a tuple of the allowed ones; ``shape``: the exact shape
    (``None`` entries: any extent); ``layout``: "contiguous" (the kernel walks the storage densely), "rows" (unit inner stride, every
    other stride and the offset whole 16-byte units: the token-stride / channel-slice views whose strides the wrapper passes on) or
    None (the wrapper makes its own copy)."""
    if t is None:
        if optional:
            return None
        _bad(fn, name, "is required")
    if not isinstance(t, torch.Tensor):
        _bad(fn, name, f"must be a tensor, got {type(t).__name__}")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        _bad(fn, name, f"has dtype {t.dtype}, expected {dtype}")
    if shape is not None and (t.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, t.shape))):
        _bad(fn, name, f"has shape {tuple(t.shape)}, expected {tuple('*' if s is None else s for s in shape)}")
    if numel is not None and t.numel() != numel:
        _bad(fn, name, f"has {t.numel()} elements, expected {numel}")
    if layout == "contiguous" and not t.is_contiguous():
        _bad(fn, name, f"must be contiguous, got strides {tuple(t.stride())}")
    if layout == "rows" and t.dim():
        vec = max(1, 16 // t.element_size())
        if (t.stride(-1) != 1 and t.shape[-1] > 1) or t.storage_offset() % vec or any(
                s % vec for s, n in zip(t.stride()[:-1], t.shape[:-1]) if n > 1):
            _bad(fn, name, f"must have unit inner stride and 16-byte rows, got strides {tuple(t.stride())} "
                           f"at offset {t.storage_offset()}")
    return t


def _same(fn, name, t, ref, optional=False):
    """Operand ``name`` is an activation of ``ref``'s dtype and shape, contiguous."""
    return _arg(fn, name, t, ref.dtype, shape=tuple(ref.shape), optional=optional)


# ----------------------------------------------------------------------------- launch context
# Everything a launch reads BESIDES its arguments lives in ONE immutable ``LaunchContext`` held in a ``contextvars.ContextVar``:
# the launch-plan divisor, the precision policy of the network that is running, the developer A/B overrides and the profiler.
# The context managers below (``plan_units``, ``f32_split``, ``tuning``) install a modified COPY for the duration of a ``with``
# block and restore the previous object on exit; nothing in this module is a mutable global.  A ContextVar is per thread (and per
# asyncio task): two threads driving two HIP streams can run two precisions at once; nested blocks on one thread compose.
class LaunchContext:
    """``plan_div``  batch-invariant plans (include/rsvld_hip.h, conventions): every launch is planned -- kernel family, tile shape,
                  split-K / split-KV -- for ONE of ``plan_div`` independent work units (images) stacked along its batch, so an
                  image's result is bit-identical however many images share the launch.  1 = plan on the whole call.
    ``policy``    the ``SplitPolicy`` of the split-precision network whose forward is running (None: not in one).
    ``tune``      developer A/B overrides -> rsvld_conv_desc.tune (every combination computes the same function); 0 = the library's choice.
    ``use_halo`` / ``halo_min_wgs`` / ``split_halo_min_wgs``   routing of eligible 3x3 convolutions through conv_halo.hip (below).
    ``split_d512_fused_min`` / ``split_attn_s_bytes``          form of the split-precision d != 64 attention (below).
    ``d64_kernel``                                             developer A/B of the d = 64 attention's two bit-identical forms.
    ``d512_kernel``                                            developer A/B of the shared-tile d = 512 attention's two bit-identical forms.
    ``profiler`` / ``profile_detail``   per-launch HIP-event bracketing (``LaunchProfiler``) and layer shapes in its group names.

    A captured hipGraph (the Stage-1 sampler's UNet forward) bakes in whatever a wrapper read here when it was captured: which
    kernel, which plan, which workspace.  ``launch_key()`` is the tuple of ALL fields that influence a launch -- every slot except
    ``NOT_IN_LAUNCH_KEY`` (``profiler``, ``profile_detail``: they bracket and name launches, they do not choose them) -- and is part
    of a capture's key.  A field added to ``__slots__`` is in the key unless it is listed there (tests/test_graph_key.py)."""

    __slots__ = ("plan_div", "policy", "tune", "use_halo", "halo_min_wgs", "split_halo_min_wgs", "split_d512_fused_min",
                 "split_attn_s_bytes", "profiler", "profile_detail", "d64_kernel", "d512_kernel")
    NOT_IN_LAUNCH_KEY = ("profiler", "profile_detail")

    def __init__(self, plan_div=1, policy=None, tune=0, use_halo=True, halo_min_wgs=256, split_halo_min_wgs=64,
                 split_d512_fused_min=2048, split_attn_s_bytes=32 << 30, profiler=None, profile_detail=False, d64_kernel=0,
                 d512_kernel=0):
        # d64_kernel: developer A/B (devtools.d64_kernel): 1 / 2 = force attn_d64b / attn_d64c (bit-identical forms)
        # d512_kernel: developer A/B (devtools.d512_kernel): 4 / 5 = force attn_d512b / attn_d512d when keys = values (bit-identical)
        # use_halo: route eligible 3x3 convs through conv_halo.hip (False: A/B against the gather kernel)
        # halo_min_wgs 256: below one workgroup per CU the 8x32-pixel halo tile under-fills the chip (measured 130 vs 334 TFLOP/s on
        #   32x32 maps): such layers use the 64x128 gather kernel with the 3-stage ring
        # split_halo_min_wgs 64: the split precision's gather kernel runs at 190-200 effective TFLOP/s where the halo kernel does
        #   385-400, and the small maps of this precision are the tiles of the tiled VAE, stacked 7-49 per launch (86 x 86 x 512:
        #   132 workgroups per planning unit, 72 x 72: 108, 86 x 64: 88): the halo tile from a quarter of a chip per unit
        # split_d512_fused_min 2048: query rows from which the fused split d = 512 kernel runs (64 per workgroup)
        # split_attn_s_bytes 32 GiB: fp32 score block of the GEMM form (P planes: as much again)
        object.__setattr__(self, "plan_div", max(1, int(plan_div)))
        for k, v in (("policy", policy), ("tune", int(tune)), ("use_halo", bool(use_halo)), ("halo_min_wgs", int(halo_min_wgs)),
                     ("split_halo_min_wgs", int(split_halo_min_wgs)), ("split_d512_fused_min", int(split_d512_fused_min)),
                     ("split_attn_s_bytes", int(split_attn_s_bytes)), ("profiler", profiler), ("profile_detail", bool(profile_detail)),
                     ("d64_kernel", int(d64_kernel)), ("d512_kernel", int(d512_kernel))):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("LaunchContext is immutable: use ops.tuning(...) / ops.plan_units(n) / ops.f32_split(policy) around the calls")

    def replace(self, **changes):
        kw = {k: getattr(self, k) for k in self.__slots__}
        bad = [k for k in changes if k not in kw]
        if bad:
            raise TypeError(f"LaunchContext has no field {bad}")
        kw.update(changes)
        return LaunchContext(**kw)

    def launch_key(self):
        """Hashable tuple of every field a launch depends on (class docstring): two contexts with equal keys issue the same launches."""
        return tuple((k, getattr(self, k)) for k in self.__slots__ if k not in self.NOT_IN_LAUNCH_KEY)


_CTX = contextvars.ContextVar("rsvld_launch_context", default=LaunchContext())


def context():
    """The LaunchContext the next launch of this thread will read."""
    return _CTX.get()


@contextlib.contextmanager
def tuning(**changes):
    """``with ops.tuning(use_halo=False, halo_min_wgs=0, tune=..., profiler=...):`` -- a modified copy of the current context for the block."""
    token = _CTX.set(_CTX.get().replace(**changes))
    try:
        yield _CTX.get()
    finally:
        _CTX.reset(token)


def set_defaults(**changes):
    """Process start-up only (rsvld_amd.devtools.apply_env, bench.py's flags): change this thread's BASE context for good."""
    _CTX.set(_CTX.get().replace(**changes))


def plan_units(n):
    """Inside ``with plan_units(n)`` every launch is planned for ONE of the ``n`` independent work units stacked along its batch."""
    return tuning(plan_div=max(1, int(n)))


# ----------------------------------------------------------------------------- split-operand precision mode
class SplitPolicy:
    """What runs at which width inside a network in the "split" precision (fp32 tensors; a matrix product = three bf16 MFMAs on
    hi + lo operands).  A policy is an ARGUMENT of the owning network (``SR_backbone.set_precision(..., policy=...)``, SR3's
    ``set_compute_dtype("split", policy=...)``), never the environment; it is part of the hipGraph key and printed by bench.py.

    ``impl``        "planes": the product path (bf16 planes + weight triples through gemm256 / conv_halo / conv_igemm);
                    "f32": round 3's on-the-fly split inside the fp32 family's simple kernels (an independent implementation of the
                    same arithmetic, kept for tests and A/B runs).
    ``f16_inputs``  the layer groups whose INPUT may be rounded to fp16 (11 significant bits) -- each measured against the reference's
                    CPU runs after 50 + 50 steps and at full depth on the device.  Their weights keep ~22 bits:
                    the layer runs as fp16 activation x fp16 weight pair [W_lo | W_hi], two MFMAs per product (dtype RSVLD_F16W2).
                      "attn"      the attention operands q, k, v, P: the 16-bit attention kernels (attn_d64c / attn_d512b)
                      "attn_out"  the input of ``to_out``: with "attn" it IS the fp16 attention output (no further rounding)
                      "ff"        the two inputs of a FeedForward: LayerNorm3's output and the GEGLU product
                      "qkv"       the inputs of to_q / to_k / to_v: LayerNorm1 / LayerNorm2's outputs (ZeroCrossAttn: its two GroupNorms)
                      "proj"      the inputs of proj_in / proj_out -- measured (+1.3e-4 after 50 steps for two GEMMs per transformer): not
                                  in the default.
                      "conv1", "conv2"  the input of a ResBlock's first / second 3x3 convolution (GroupNorm + SiLU outputs; NOT conv_in,
                                  the Down / Upsample and ZeroSFT convolutions or the output convolution).  Every convolution input in
                                  fp16 is 3.4e-3 on the CPU restatement; experiments only: on the reduced-depth goldens the first
                                  convolution's input costs +1.5e-4 after 50 steps and the second's +3.2e-4, but at full network depth the
                                  first alone ends at 1.2-1.7e-3 -- the reason the full-depth test exists.
                    Measured after 50 Stage-2 steps against the reference's CPU run (tools/tolerance_check.py, round 5, max / mean):
                    ("attn",) 2.5e-4 / 3.8e-5; + attn_out + ff 3.5e-4 / 4.6e-5; + qkv 3.5e-4 / 5.3e-5 (the default); + conv1 5.0e-4 / 6.7e-5
                    on the reduced-depth goldens but 1.2e-3 / 1.7e-3 (cache off / 0.3) at FULL depth against the fp32 family
                    (tests/test_gpu_fulldepth.py): outside the bar, rejected; qkv + conv2 6.6e-4 / 9.7e-5; qkv + conv1 + conv2 6.9e-4 / 9.3e-5;
                    qkv + proj 4.8e-4 / 6.5e-5.
    ``f16_weights`` the GEMM groups whose WEIGHTS are rounded to fp16 as well -- fp16 activation x fp16 weight, ONE MFMA per product, the plain
                    gemm256 / conv_igemm kernels -- where the input already is fp16 (default: all four wherever ``f16_inputs`` allows):
                      "qkv"       to_q / to_k / to_v (fp16 out: the attention operands)
                      "geglu"     the GEGLU projection of a FeedForward (fp16 out)
                      "attn_out", "ff_out"   to_out / ff.net.2 (fp32 out + fp32 residual: dtype RSVLD_F16W1)
                    A rounded weight is the SAME perturbation at every step, so this was expected to cost more than a rounded activation; measured
                    it does not: after 50 steps on the reduced-depth goldens 3.5e-4 / 5.3e-5 (every weight a pair) -> 5.3e-4 / 6.3e-5 (qkv + geglu) ->
                    4.5e-4 / 7.0e-5 (all four: the default; single groups scatter between 4.5e-4 and 7.8e-4 in the maximum, 6.3-7.5e-5 in the
                    mean); at FULL depth against the fp32 family 2.9e-4 -> 5.4e-4 (cache off), 4.0e-4 -> 4.9e-4 (0.3), means 3.9e-5 / 4.6e-5, every
                    cache decision equal (tools/tolerance_check.py, tools/fulldepth_check.py; the residual stream, the norms, proj_in / proj_out and
                    every convolution stay fp32 / three-MFMA).  16.7 -> 10.5 s of GEMM time per 4096^2 image.
                    The convolutions are different: their weights rounded to fp16 (emulated through the triples of fp16(W), round 5) end at
                    1.8e-3 on the goldens and 2.6e-3 / 2.3e-3 at full depth -- no two-MFMA form of the 3x3 layers on fp16 planes x fp16 weights.
    ``q8_convs``    (round 6) the ResBlock convolutions ("conv1", "conv2": the two 3x3 layers behind a GroupNorm + SiLU) that keep BOTH operands
                    at ~22 bits but spend fewer matrix cycles on them: x w = f16(x) f16(w) + x_lo w_hi + x_hi w_lo with the two cross terms
                    (2^-11 of the product) contracted in e4m3 on the block-scaled matrix instruction (dtype RSVLD_F16Q8: per 32 channels and tap
                    two fp16 MFMAs + one scaled MFMA instead of six bf16 MFMAs).  Emulated at full depth over 50 steps before the kernel was
                    written: mean distance from the fp32 family +3.5 %, maxima 5.8e-4 / 5.1e-4, every cache decision unchanged
                    (profiles/r06_conv_lo8_emulation.txt).  Default (``None``): in the product path with the four transformer groups of the
                    shipped composition ("attn", "attn_out", "ff", "qkv") in ``f16_inputs``, every group of ``Q8_GROUPS`` that ``f16_inputs``
                    does not already round to fp16 -- both in the shipped composition; none elsewhere (the VAE: real SDXL-VAE activations
                    leave the fp16 range).  An explicit ``q8_convs`` that names a group of ``f16_inputs`` is an error.
                    Range: the e4m3 cross terms saturate (include/rsvld_hip.h, RSVLD_HQ8_SX_*): x_lo from |x| ~ 64, x_hi above |x| = 112."""

    __slots__ = ("impl", "f16_inputs", "f16_weights", "q8_convs")
    GROUPS = ("attn", "attn_out", "ff", "qkv", "proj", "conv1", "conv2")
    WEIGHT_GROUPS = ("qkv", "geglu", "attn_out", "ff_out")
    Q8_GROUPS = ("conv1", "conv2")

    def __init__(self, impl="planes", f16_inputs=("attn", "attn_out", "ff", "qkv"), f16_weights=None, q8_convs=None):
        if q8_convs is None:        # the default: the ResBlock convolutions not rounded to fp16, in the shipped composition of the UNets only
            q8_convs = (tuple(g for g in self.Q8_GROUPS if g not in f16_inputs)
                        if (impl == "planes" and {"attn", "attn_out", "ff", "qkv"} <= set(f16_inputs)) else ())
        bad = [g for g in q8_convs if g not in self.Q8_GROUPS]
        if bad:
            raise ValueError(f"SplitPolicy.q8_convs {bad}: one of {self.Q8_GROUPS}")
        if set(q8_convs) & set(f16_inputs):
            raise ValueError("SplitPolicy: a convolution's input is either rounded to fp16 (f16_inputs) or kept with e4m3 cross terms (q8_convs)")
        if q8_convs and impl != "planes":
            raise ValueError("SplitPolicy.q8_convs exists in the product path (impl \"planes\") only")
        self.q8_convs = frozenset(q8_convs)
        if f16_weights is None:     # the default: every transformer GEMM whose input is fp16
            f16_weights = tuple(g for g, i in (("qkv", "qkv"), ("geglu", "ff"), ("attn_out", "attn_out"), ("ff_out", "ff")) if i in f16_inputs and impl == "planes")
        bad = [g for g in f16_weights if g not in self.WEIGHT_GROUPS]
        if bad:
            raise ValueError(f"SplitPolicy.f16_weights {bad}: one of {self.WEIGHT_GROUPS}")
        self.f16_weights = frozenset(f16_weights)
        if impl not in ("planes", "f32"):
            raise ValueError(f"SplitPolicy.impl {impl!r}: planes or f32")
        bad = [g for g in f16_inputs if g not in self.GROUPS]
        if bad:
            raise ValueError(f"SplitPolicy.f16_inputs {bad}: one of {self.GROUPS}")
        self.impl, self.f16_inputs = impl, frozenset(f16_inputs)
        if self.f16_inputs - {"attn"} and "attn" not in self.f16_inputs:
            raise ValueError("SplitPolicy: fp16 layer inputs go with fp16 attention operands (\"attn\")")
        if self.f16_inputs and impl != "planes":
            raise ValueError("SplitPolicy: fp16 layer inputs exist in the product path (impl \"planes\") only")
        need = {"qkv": "qkv", "geglu": "ff", "attn_out": "attn_out", "ff_out": "ff"}
        bad = [g for g in self.f16_weights if need[g] not in self.f16_inputs]
        if bad:
            raise ValueError(f"SplitPolicy.f16_weights {bad}: a layer's weights are rounded to fp16 only where its input is (f16_inputs)")

    def key(self):
        return (self.impl, tuple(sorted(self.f16_inputs)), tuple(sorted(self.f16_weights)), tuple(sorted(self.q8_convs)))

    def describe(self):
        return {"impl": self.impl, "f16_inputs": sorted(self.f16_inputs), "f16_weights": sorted(self.f16_weights), "q8_convs": sorted(self.q8_convs)}

    def __eq__(self, o):
        return isinstance(o, SplitPolicy) and self.key() == o.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return (f"SplitPolicy(impl={self.impl!r}, f16_inputs={sorted(self.f16_inputs)}, f16_weights={sorted(self.f16_weights)}, "
                f"q8_convs={sorted(self.q8_convs)})")


UNET_POLICY = SplitPolicy()                                   # the UNets / ControlNet of Stage 2
ALL_SPLIT = SplitPolicy(f16_inputs=(), f16_weights=())                        # every product in three MFMAs, attention in the split kernels
VAE_POLICY = ALL_SPLIT                                        # the VAE (its single-head attentions are a third of the Stage-2 distance in fp16)

# Inside ``with f32_split(policy)`` the matrix products of fp32 tensors run in the split precision under that policy
# (``True`` = UNET_POLICY, ``False`` / ``None`` = off).  Entered by the owning network around its forward.
def f32_split(on):
    return tuning(policy=UNET_POLICY if on is True else (on if isinstance(on, SplitPolicy) else None))


def _policy():
    return _CTX.get().policy


def _split_fast():
    pol = _CTX.get().policy
    return pol is not None and pol.impl == "planes"


def precision_token():
    """Hashable name of the precision the current call runs in (None outside a split-precision network): cached intermediate tensors
    (the text context's K | V) are keyed on it."""
    pol = _CTX.get().policy
    return None if pol is None else pol.key()


def f16_group(group):
    """Does the current policy hand the inputs of layer group ``group`` over as fp16?"""
    if group is None:
        return False
    pol = _CTX.get().policy
    return pol is not None and pol.impl == "planes" and group in pol.f16_inputs


def q8_group(group):
    """Does the current policy run the 3x3 convolution behind norm group ``group`` with e4m3 cross terms (RSVLD_F16Q8)?"""
    if group is None:
        return False
    pol = _CTX.get().policy
    return pol is not None and pol.impl == "planes" and group in pol.q8_convs


class Q8Rows:
    """An activation in the RSVLD_F16Q8 row format: ``t`` is an fp16-typed tensor ``[B, H, W, 2, C]`` whose first plane is fp16(x) and whose
    second plane holds, per 32 channels, 64 bytes of e4m3 cross-term operands (include/rsvld_hip.h); only the halo convolution reads it."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    @property
    def shape(self):
        s = self.t.shape
        return tuple(s[:-2]) + (s[-1],)


class Planes:
    """The split form of an fp32 tensor ``[..., C]``: ``t`` is a bf16 tensor ``[..., 2, C]`` with plane 0 = lo, plane 1 = hi
    (hi = bf16(v), lo = bf16(v - hi)); contiguous planes are rows ``lo(C) | hi(C)``, the layout RSVLD_SPLIT kernels read and write.
    A tensor that only feeds matrix products travels like this (same bytes as fp32, nothing lost that the product would keep).
    Duck-types the few tensor members the network code touches between ops: shape, reshape, last-dim slices."""

    __slots__ = ("t", "_gn_part", "_nhwc")
    dtype = torch.float32      # the LOGICAL dtype: code that asks ``x.dtype == torch.float32`` means "the fp32 / split families"

    def __init__(self, t):
        self.t = t

    @property
    def shape(self):
        return tuple(self.t.shape[:-2]) + (self.t.shape[-1],)

    @property
    def device(self):
        return self.t.device

    @property
    def is_cuda(self):
        return self.t.is_cuda

    def dim(self):
        return self.t.dim() - 1

    def numel(self):
        return self.t.numel() // 2

    def element_size(self):
        return 4

    def is_contiguous(self):
        return self.t.is_contiguous()

    def contiguous(self):
        return self if self.t.is_contiguous() else Planes(self.t.contiguous())

    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        return Planes(self.t.reshape(*shape[:-1], 2, self.t.shape[-1] if shape[-1] == -1 else shape[-1]))

    def __getitem__(self, idx):
        if not isinstance(idx, tuple):
            idx = (idx,)
        if Ellipsis in idx:
            i = idx.index(Ellipsis)
            idx = idx[:i] + (slice(None),) * (self.dim() - (len(idx) - 1)) + idx[i + 1:]
        idx = idx + (slice(None),) * (self.dim() - len(idx))
        return Planes(self.t[idx[:-1] + (slice(None), idx[-1])])

    def index_select(self, dim, index):
        return Planes(self.t.index_select(dim, index))

    def float(self):
        return self.f32()

    def f32(self):
        """-> the fp32 tensor hi + lo (rsvld_merge_planes)."""
        t = self.t.contiguous()
        Cc = t.shape[-1]
        out = torch.empty(tuple(t.shape[:-2]) + (Cc,), device=t.device, dtype=torch.float32)
        L.check(L.load().rsvld_merge_planes(_ptr(t), _ptr(out), t.numel() // (2 * Cc), Cc, _stream()), "rsvld_merge_planes")
        if out.dim() == 4:
            out._nhwc = True
        return out


def to_planes(x):
    """fp32 ``[..., C]`` (C % 8 == 0, contiguous) -> Planes (rsvld_split_planes); a Planes passes through."""
    if isinstance(x, Planes):
        return x
    _arg("to_planes", "x", x, torch.float32)
    if x.dim() < 1 or x.shape[-1] % 8:
        _bad("to_planes", "x", f"needs C % 8 == 0, got shape {tuple(x.shape)}")
    _need_gpu(x)
    Cc = x.shape[-1]
    t = torch.empty(tuple(x.shape[:-1]) + (2, Cc), device=x.device, dtype=torch.bfloat16)
    _launch("split_planes", 0.0, 8.0 * x.numel(), lambda: L.check(L.load().rsvld_split_planes(_ptr(x), _ptr(t), x.numel() // Cc, Cc, _stream()),
                                                                  "rsvld_split_planes"))
    return Planes(t)


def as_f32(x):
    return x.f32() if isinstance(x, Planes) else x


def maybe_planes(x):
    """In the split precision: the planes of an fp32 tensor that SEVERAL matrix products are about to read (split it once instead
    of once per product); any other mode / tensor passes through."""
    if _split_fast() and not isinstance(x, Planes) and x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 8 == 0:
        return to_planes(x)
    return x


# ----------------------------------------------------------------------------- launch profiling
class LaunchProfiler:
    """Brackets every C-ABI launch with HIP events on the launch stream (torch's current stream is
    the stream the kernels are enqueued on) and accumulates time / algorithmic FLOPs per kernel."""

    def __init__(self):
        self.records = []

    def run(self, name, flops, nbytes, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.records.append((name, flops, nbytes, e0, e1))
        return out

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, flops, nbytes, e0, e1 in self.records:
            r = agg.setdefault(name, {"name": name, "ms": 0.0, "n": 0, "flops": 0.0, "bytes": 0.0})
            r["ms"] += e0.elapsed_time(e1)
            r["n"] += 1
            r["flops"] += flops
            r["bytes"] += nbytes
        return agg


def set_profiler(p):
    """Bracket every launch of this thread from now on (``None``: stop).  Scoped form: ``with ops.tuning(profiler=p):``."""
    set_defaults(profiler=p)


def _launch(name, flops, nbytes, fn):
    prof = _CTX.get().profiler
    if prof is None:
        return fn()
    return prof.run(name, flops, nbytes, fn)


# ----------------------------------------------------------------------------- weights
class PackedConv:
    """K-major 16-bit weights of a Conv2d / Linear: ``w[Cout_p, KH*KW*Cin_p]``, bias fp32."""

    __slots__ = ("w", "bias", "cin", "cout", "cin_p", "cout_p", "kh", "kw", "geglu", "w3", "w2", "w1", "wq8")

    def __init__(self, w, bias, cin, cout, cin_p, cout_p, kh, kw, geglu=False):
        self.w, self.bias = w, bias
        self.w3 = None     # split product path: bf16 triples [Cout_p][KH*KW][W_hi | W_lo | W_hi], packed on first use from the fp32 ``w``
        self.w1 = None     # the fp32 ``w`` rounded to fp16 (SplitPolicy.f16_weights: fp16 activation x fp16 weight, one MFMA), likewise
        self.w2 = None     # fp16 pairs [Cout_p][KH*KW][W_lo | W_hi] (dtype RSVLD_F16W2: fp16 activations), likewise
        self.wq8 = None    # RSVLD_F16Q8 rows [Cout_p][KH*KW][fp16(w) | e4m3 cross-term blocks], likewise
        self.cin, self.cout, self.cin_p, self.cout_p = cin, cout, cin_p, cout_p
        self.kh, self.kw, self.geglu = kh, kw, geglu


def pack_conv(weight, bias, dtype, device, cin_split=None, geglu=False):
    """fp32 ``[Cout, Cin, KH, KW]`` (or Linear ``[Cout, Cin]``) -> PackedConv on ``device``.

    ``cin_split=(C1, C2)``: the layer consumes the concatenation of two NHWC tensors whose channel
    counts are padded separately to multiples of 8.  ``geglu``: rows are re-ordered so that value j
    and gate j (rows j and j + Cout/2 of the reference weight, sgm/modules/attention.py:84-96)
    become adjacent output channels 2j, 2j+1.
    """
    # (the re-layout runs where the master weights live: on the device for a loaded network -- no 15 GB round trip over PCIe and no
    #  host-side permute of 3.9 B values when a precision is switched -- on the host for weights that are still there)
    w = weight.detach().to(torch.float32)
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    b = None if bias is None else bias.detach().to(device=w.device, dtype=torch.float32)
    if geglu:
        half = cout // 2
        idx = torch.stack([torch.arange(half), torch.arange(half) + half], 1).reshape(-1).to(w.device)
        w = w[idx]
        b = None if b is None else b[idx]
    parts = [cin] if cin_split is None else list(cin_split)
    assert sum(parts) == cin
    w = w.permute(0, 2, 3, 1)  # [Cout, KH, KW, Cin]
    chunks, off = [], 0
    for c in parts:
        blk = w[..., off:off + c]
        if pad8(c) != c:
            blk = torch.nn.functional.pad(blk, (0, pad8(c) - c))
        chunks.append(blk)
        off += c
    w = torch.cat(chunks, dim=-1)
    cin_p = w.shape[-1]
    cout_p = pad8(cout) if not geglu else (cout + 15) // 16 * 16
    if cout_p != cout:
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cout_p - cout))
        if b is not None:
            b = torch.nn.functional.pad(b, (0, cout_p - cout))
    w = w.reshape(cout_p, kh * kw * cin_p).contiguous().to(device=device, dtype=dtype)
    b = None if b is None else b.contiguous().to(device)
    return PackedConv(w, b, cin, cout, cin_p, cout_p, kh, kw, geglu)


# ----------------------------------------------------------------------------- conv / linear
def conv2d(x, pc, *, x2=None, stride=1, pad=None, upsample=False, rowvec=None, residual=None,
           out_f32=False, act=L.ACT_NONE, alpha=1.0, beta=1.0, norm=None, stats=False, out_planes=False, out_group=None, norm_group=None,
           group=None):
    """NHWC convolution.  ``pad`` = int or (top, left, bottom, right).

    ``norm=(gamma, beta, groups, eps, silu)``: a GroupNorm(+SiLU) over the input ([x | x2]) precedes the
    conv.  For 3x3/stride-1 convs it is FUSED into the conv's input staging (rsvld_conv3x3_halo_nhwc): one
    statistics pass over x, no normalised tensor in HBM.  Otherwise it runs as its own kernels first.

    ``stats=True``: the caller will feed the output to a GroupNorm; when the halo kernel runs it also writes
    per-tile per-channel (sum, sumsq) of the output from its epilogue and attaches them to the returned tensor
    (``_gn_part``), so the consumer's ``norm=`` needs no statistics pass at all.

    ``out_planes=True`` (honoured in the split precision only, ignored otherwise): the output only feeds another matrix
    product (q|k|v, GEGLU, ...) and is returned as ``Planes`` -- or as fp16 when the policy hands the inputs of its consumer's
    layer group ``out_group`` over in fp16 (``SplitPolicy.f16_inputs``).

    fp16 ``x`` with weights packed in fp32 (a network in the split precision whose policy rounds this layer's input to fp16, or SR3's
    compute dtype "w2"): dtype RSVLD_F16W2, fp16 activation x fp16 weight pair [W_lo | W_hi], two MFMAs per product; in a
    split-precision network the output is fp32 (+ fp32 residual) unless ``out_planes`` asks for the fp16 hand-over."""
    _conv_operands("conv2d", x, pc, x2, stride, pad, upsample, rowvec, residual, out_f32, act, norm, out_planes)
    _need_gpu(x, x2, pc.w, rowvec, residual)
    ctx = _CTX.get()
    if isinstance(x, Planes) or (x.dtype == torch.float32 and _split_fast()):
        return _conv2d_split(x, pc, x2=x2, stride=stride, pad=pad, upsample=upsample, rowvec=rowvec, residual=residual,
                             act=act, alpha=alpha, beta=beta, norm=norm, stats=stats, out_planes=out_planes, out_group=out_group,
                             norm_group=norm_group, group=group)
    if x.dtype == torch.float32:
        return _conv2d_f32(x, pc, x2=x2, stride=stride, pad=pad, upsample=upsample, rowvec=rowvec, residual=residual,
                           act=act, alpha=alpha, beta=beta, norm=norm)
    w2 = pc.w.dtype == torch.float32         # fp32 masters under a 16-bit activation: the weight-pair form (fp16 only: _conv_operands)
    w1res = False
    if w2 and _split_fast():
        out_f32 = not out_planes
        # the layer's weight group (SplitPolicy.f16_weights): named by the caller, or implied by the consumer of an fp16 output
        wg = group if group is not None else ({"attn": "qkv", "ff": "geglu"}.get(out_group) if not out_f32 else None)
        if wg is not None and ctx.policy is not None and wg in ctx.policy.f16_weights:
            if out_f32:
                if pc.kh != 1 or pc.kw != 1 or x2 is not None:
                    raise L.RsvldError(f"conv2d: SplitPolicy.f16_weights {wg!r} with an fp32 output is a Linear layer's form (RSVLD_F16W1)")
                w1res = True  # fp16 x fp16, ONE MFMA per product, fp32 out + fp32 residual (dtype RSVLD_F16W1)
            else:
                w2 = False    # the plain fp16 kernels
    wt = _w1(pc) if w1res else _w2(pc) if w2 else (_w1(pc) if pc.w.dtype == torch.float32 else pc.w)
    B, H, W, Cin = x.shape
    Cin2 = 0 if x2 is None else x2.shape[-1]
    geo = _conv_geometry(x.shape, pc, stride, pad, upsample, act)
    Ho, Wo, c_out = geo[2:]
    out = torch.empty((B, Ho, Wo, c_out), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    d = _conv_desc(x.shape, Cin2, pc, geo, L.F16W1 if w1res else L.F16W2 if w2 else _dt(x), int(out_f32), stride=stride,
                   upsample=upsample, act=act, alpha=alpha, beta=beta, x=x, x2=x2, w=wt, rowvec=rowvec, residual=residual, out=out)
    sfx = "_w1" if w1res else "_w2" if w2 else ""
    lib = L.load()
    plan, rc = _conv_plan(lib, d)
    # policy: the halo kernel where the library has one for the layer and its grid fills the chip; no fused norm before an Upsample conv
    halo = ctx.use_halo and plan.halo_bn != 0 and plan.halo_wgs >= ctx.halo_min_wgs and not (upsample and norm is not None)
    if norm is not None and not halo:   # unfused: normalise into a (single) tensor, then convolve it
        gamma, nbeta, groups, eps, silu = norm
        xn = group_norm(x, gamma, nbeta, groups, eps, x2=x2, silu=silu)
        return conv2d(xn, pc, stride=stride, pad=pad, upsample=upsample, rowvec=rowvec, residual=residual,
                      out_f32=out_f32, act=act, alpha=alpha, beta=beta, stats=stats, out_planes=out_planes, out_group=out_group, group=group)
    esz = x.element_size()
    flops = 2.0 * B * Ho * Wo * pc.cout * pc.cin * pc.kh * pc.kw
    nbytes = (x.numel() + (0 if x2 is None else x2.numel()) + wt.numel()) * esz + out.numel() * out.element_size() \
        + (0 if residual is None else residual.numel() * residual.element_size())
    if halo:
        ab, silu = None, 0
        if norm is not None:
            gamma, nbeta, groups, eps, silu = norm
            ab = _gn_ab_from_partials(x, x2, gamma, nbeta, groups, eps)     # statistics came with the producers' epilogues
            if ab is None:
                ws = torch.empty(lib.rsvld_groupnorm_ws_bytes(B, H * W, Cin + Cin2, groups), device=x.device, dtype=torch.uint8)
                ab = torch.empty((B, Cin + Cin2, 2), device=x.device, dtype=torch.float32)
                _launch("groupnorm_stats(3 kernels)", 0.0, x.numel() * esz + (0 if x2 is None else x2.numel() * esz),
                        lambda: L.check(lib.rsvld_groupnorm_scale_shift(_ptr(x), _ptr(x2), _ptr(gamma), _ptr(nbeta), _ptr(ab), B,
                                                                        H * W, Cin, Cin2, groups, eps, _dt(x), _ptr(ws), _stream()),
                                        "rsvld_groupnorm_scale_shift"))
        _halo_launch(f"conv_halo_{plan.halo_bn}" + sfx + _detail(B, Ho, Wo, Cin, Cin2, pc, stride, upsample), flops, nbytes, d, out, ab, silu,
                     plan.halo_stat_tiles if stats and (w2 or not out_f32) else 0)
        return out
    L.check(rc, "rsvld_plan_conv")
    variant = "gemm_256x256" if plan.gemm256 else f"conv_igemm_{plan.bm}x{plan.bn}"   # the kernel that runs, tune bits included
    _launch(variant + sfx + _detail(B, Ho, Wo, Cin, Cin2, pc, stride, upsample), flops, nbytes, lambda: L.check(lib.rsvld_conv2d_nhwc(C.byref(d), _stream()), "rsvld_conv2d_nhwc"))
    if out_f32 and out.dim() == 4:
        out._nhwc = True     # an fp32 4-d tensor is otherwise taken for NCHW by the VAE's input adapter
    return out


def _conv_operands(fn, x, pc, x2, stride, pad, upsample, rowvec, residual, out_f32, act, norm, out_planes):
    """The contract of every operand of conv2d / linear: NHWC ``x`` (16-bit, fp32 or contiguous planes) and ``x2`` of the same kind and
    pixels, weights packed in ``x``'s type (or fp32: the weight-pair form under fp16, the fp32 / split families), fp32 bias and norm
    affine of the layer's channels, fp32 ``rowvec [B, Cout]`` with unit inner stride, ``residual`` of the output's shape and type."""
    if isinstance(x, Planes):
        _arg(fn, "x", x.t, torch.bfloat16, shape=(None,) * 3 + (2, None))
    else:
        _arg(fn, "x", x, _ACT, shape=(None,) * 4)
    f32 = isinstance(x, Planes) or x.dtype == torch.float32
    B, H, W, Cin = x.shape
    Cin2 = 0
    if isinstance(x2, Planes):
        if not f32:
            _bad(fn, "x2", "is planes under a 16-bit x")
        _arg(fn, "x2", x2.t, torch.bfloat16, shape=(B, H, W, 2, None))
    elif x2 is not None:
        _arg(fn, "x2", x2, torch.float32 if f32 else x.dtype, shape=(B, H, W, None))
    if x2 is not None:
        Cin2 = x2.shape[-1]
    wdt = torch.float32 if f32 else ((torch.float16, torch.float32) if x.dtype == torch.float16 else x.dtype)
    _arg(fn, "pc.w", pc.w, wdt, shape=(pc.cout_p, pc.kh * pc.kw * pc.cin_p))
    _arg(fn, "pc.bias", pc.bias, torch.float32, shape=(pc.cout_p,), optional=True)
    if Cin + Cin2 != pc.cin_p:
        _bad(fn, "x", f"has {Cin}+{Cin2} channels, the packed weights {pc.cin_p}")
    if norm is not None:
        _arg(fn, "norm gamma", norm[0], torch.float32, shape=(Cin + Cin2,), optional=True)
        _arg(fn, "norm beta", norm[1], torch.float32, shape=(Cin + Cin2,), optional=True)
    _arg(fn, "rowvec", rowvec, torch.float32, shape=(B, pc.cout_p), layout=None, optional=True)
    if rowvec is not None and rowvec.stride(1) != 1:
        _bad(fn, "rowvec", f"must have unit inner stride, got strides {tuple(rowvec.stride())}")
    if residual is not None:
        shape = (B,) + _conv_geometry(x.shape, pc, stride, pad, upsample, act)[2:]
        if f32:
            rdt = torch.float32
        elif pc.w.dtype == torch.float32 and _split_fast():   # the weight-pair form in a split-precision network
            rdt = torch.float16 if out_planes else torch.float32
        else:
            rdt = torch.float32 if out_f32 else x.dtype
        _arg(fn, "residual", residual, rdt, shape=shape)


def _conv_geometry(shape, pc, stride, pad, upsample, act):
    """Where the output of ``pc`` over an NHWC input of ``shape`` lies -> ``(pt, pl, Ho, Wo, c_out)``: ``pad`` = None (``kh // 2``), an int
    or (top, left, bottom, right); ``upsample`` doubles the input first; GEGLU halves the channels.  Integer arithmetic only."""
    H, W = shape[1], shape[2]
    if pad is None:
        pad = pc.kh // 2
    pt, pl, pb, pr = (pad,) * 4 if isinstance(pad, int) else pad
    Hin, Win = (2 * H, 2 * W) if upsample else (H, W)
    Ho = (Hin + pt + pb - pc.kh) // stride + 1
    Wo = (Win + pl + pr - pc.kw) // stride + 1
    return pt, pl, Ho, Wo, pc.cout_p // 2 if act == L.ACT_GEGLU else pc.cout_p


def _conv_desc(shape, Cin2, pc, geo, dtype, out_f32, *, stride=1, upsample=False, act=L.ACT_NONE, alpha=1.0, beta=1.0, x=None, x2=None,
               w=None, rowvec=None, residual=None, out=None, plan_div=None, tune=None):
    """The rsvld_conv_desc (include/rsvld_hip.h; field by field L.ConvDesc) of ``pc`` on an input of ``shape`` = ``[B, H, W, Cin]`` (+ ``Cin2``
    channels of ``x2``) with the geometry ``geo`` of ``_conv_geometry``: the only place that fills one.  Absent tensors are null pointers
    (nothing here needs a device).  ``dtype`` / ``out_f32``: RSVLD_* operand form and output code (0: the activation's type, 1: fp32,
    2: fp16 from RSVLD_SPLIT).  ``rowvec [B, Cout]`` may be a view with a row stride (one row: the stride is never used).
    ``plan_div`` / ``tune``: the launch context's unless the caller plans on the whole call / sets its own bits."""
    ctx = _CTX.get()
    B, H, W, Cin = shape
    pt, pl, Ho, Wo, _ = geo
    ptr = lambda t: None if t is None else t.data_ptr()
    return L.ConvDesc(
        x=ptr(x), x2=ptr(x2), w=ptr(w), bias=ptr(pc.bias), rowvec=ptr(rowvec), residual=ptr(residual), out=ptr(out),
        B=B, H=H, W=W, Cin=Cin, Cin2=Cin2, Cout=pc.cout_p, KH=pc.kh, KW=pc.kw, stride=stride, pad_t=pt, pad_l=pl, Ho=Ho, Wo=Wo,
        upsample=int(upsample), dtype=dtype, out_f32=out_f32, act=act, alpha=alpha, beta=beta,
        rowvec_stride=0 if rowvec is None else (rowvec.stride(0) if B > 1 else pc.cout_p),
        plan_div=ctx.plan_div if plan_div is None else plan_div, tune=ctx.tune if tune is None else tune)


def _conv_plan(lib, d):
    """rsvld_plan_conv (include/rsvld_hip.h; ``lib``: L.load()) of descriptor ``d`` -> ``(L.ConvPlan, rc)``: the library's own launch plan, asked once per
    layer instead of restated here.  ``halo_bn`` (0: no halo kernel for this layer), ``halo_wgs`` (its workgroups per planning unit, for
    ``halo_min_wgs`` / ``split_halo_min_wgs``) and ``halo_stat_tiles`` (rows of its epilogue statistics) hold whatever ``rc`` says;
    ``rc``: what rsvld_conv2d_nhwc would return before launching, and with 0 ``gemm256`` or the implicit-GEMM tile ``bm`` x ``bn``.
    Host arithmetic only: absent tensors may be null pointers where only the halo fields are read."""
    plan = L.ConvPlan()
    return plan, lib.rsvld_plan_conv(d, plan)     # (ctypes passes a structure by reference where the argument type is a pointer to it)


def _halo_launch(name, flops, nbytes, d, out, ab, silu, ntiles):
    """rsvld_conv3x3_halo_nhwc on descriptor ``d`` (``ab`` / ``silu``: the fused GroupNorm of its input, or None / 0).  ``ntiles``: 0, or
    the plan's ``halo_stat_tiles``: the epilogue writes per-tile per-channel fp64 (sum, sumsq) of the output, attached to ``out`` as
    ``_gn_part`` for the consumer's ``norm=``."""
    part_out = None
    if ntiles:
        part_out = torch.empty((d.B, ntiles, d.Cout, 2), device=out.device, dtype=torch.float64)
    _launch(name, flops, nbytes, lambda: L.check(L.load().rsvld_conv3x3_halo_nhwc(C.byref(d), _ptr(ab), int(silu), _ptr(part_out), _stream()),
                                                 "rsvld_conv3x3_halo_nhwc"))
    if part_out is not None:
        out._gn_part = (part_out, ntiles)


def _conv2d_f32(x, pc, *, x2, stride, pad, upsample, rowvec, residual, act, alpha, beta, norm):
    """fp32 NHWC convolution with fp32 packed weights (rsvld_conv2d_nhwc_f32); a ``norm=`` GroupNorm runs first, unfused."""
    if norm is not None:
        gamma, nbeta, groups, eps, silu = norm
        x, x2 = group_norm(x, gamma, nbeta, groups, eps, x2=x2, silu=silu), None
    B = x.shape[0]
    geo = _conv_geometry(x.shape, pc, stride, pad, upsample, act)
    Ho, Wo, c_out = geo[2:]
    out = torch.empty((B, Ho, Wo, c_out), device=x.device, dtype=torch.float32)
    split = _policy() is not None
    d = _conv_desc(x.shape, 0 if x2 is None else x2.shape[-1], pc, geo, L.F32, 1, stride=stride, upsample=upsample, act=act, alpha=alpha,
                   beta=beta, x=x, x2=x2, w=pc.w, rowvec=rowvec, residual=residual, out=out, plan_div=1,
                   tune=L.TUNE_F32_SPLIT if split else 0)
    flops = 2.0 * B * Ho * Wo * pc.cout * pc.cin * pc.kh * pc.kw
    nbytes = 4.0 * (x.numel() + pc.w.numel() + out.numel() + (0 if residual is None else residual.numel()))
    _launch("conv_f32_split" if split else "conv_f32", flops, nbytes, lambda: L.check(L.load().rsvld_conv2d_nhwc_f32(C.byref(d), _stream()),
                                                                                    "rsvld_conv2d_nhwc_f32"))
    out._nhwc = True     # an fp32 4-d tensor is otherwise taken for NCHW by the VAE's input adapter
    return out


def _w3(pc):
    """bf16 weight triples of a PackedConv (fp32 K-major ``w``), packed once on the device."""
    if pc.w3 is None:
        if pc.w.dtype != torch.float32:
            raise L.RsvldError("split precision: weights must be packed in fp32 (the owning network's compute_dtype)")
        taps = pc.kh * pc.kw
        w3 = torch.empty((pc.cout_p, taps * 3 * pc.cin_p), device=pc.w.device, dtype=torch.bfloat16)
        L.check(L.load().rsvld_split_pack_weights(_ptr(pc.w), _ptr(w3), pc.cout_p, taps, pc.cin_p, _stream()), "rsvld_split_pack_weights")
        pc.w3 = w3
    return pc.w3


def _w1(pc):
    """The fp32 K-major ``w`` of a PackedConv rounded to fp16 (SplitPolicy.f16_weights), once."""
    if pc.w1 is None:
        pc.w1 = pc.w.half()
    return pc.w1


def _w2(pc):
    """fp16 weight pairs [W_lo | W_hi] of a PackedConv (fp32 K-major ``w``), packed once on the device."""
    if pc.w2 is None:
        if pc.w.dtype != torch.float32:
            raise L.RsvldError("weight pairs: weights must be packed in fp32 (the owning network's compute_dtype)")
        taps = pc.kh * pc.kw
        w2 = torch.empty((pc.cout_p, taps * 2 * pc.cin_p), device=pc.w.device, dtype=torch.float16)
        L.check(L.load().rsvld_pack_weight_pairs(_ptr(pc.w), _ptr(w2), pc.cout_p, taps, pc.cin_p, _stream()), "rsvld_pack_weight_pairs")
        pc.w2 = w2
    return pc.w2


def _wq8(pc):
    """RSVLD_F16Q8 weight rows of a PackedConv (fp32 K-major ``w``, input channels a multiple of 32), packed once on the device."""
    if pc.wq8 is None:
        if pc.w.dtype != torch.float32 or pc.cin_p % 32:
            raise L.RsvldError("e4m3 cross-term weights: fp32-packed weights with a multiple of 32 input channels expected")
        taps = pc.kh * pc.kw
        wq = torch.empty((pc.cout_p, taps * 2 * pc.cin_p), device=pc.w.device, dtype=torch.float16)
        L.check(L.load().rsvld_pack_weight_hq8(_ptr(pc.w), _ptr(wq), pc.cout_p, taps, pc.cin_p, _stream()), "rsvld_pack_weight_hq8")
        pc.wq8 = wq
    return pc.wq8


def to_q8rows(x):
    """fp32 ``[..., C]`` (C % 32 == 0, contiguous) -> Q8Rows (rsvld_split_hq8): the activation format of RSVLD_F16Q8."""
    _arg("to_q8rows", "x", x, torch.float32)
    if x.dim() < 1 or x.shape[-1] % 32:
        _bad("to_q8rows", "x", f"needs a multiple of 32 channels, got shape {tuple(x.shape)}")
    _need_gpu(x)
    Cc = x.shape[-1]
    t = torch.empty(tuple(x.shape[:-1]) + (2, Cc), device=x.device, dtype=torch.float16)
    _launch("split_q8", 0.0, 8.0 * x.numel(), lambda: L.check(L.load().rsvld_split_hq8(_ptr(x), _ptr(t), x.numel() // Cc, Cc, _stream()),
                                                            "rsvld_split_hq8"))
    return Q8Rows(t)


def _q8_conv_eligible(B, H, W, Cc, pc, stride, pad, upsample, act, out_planes):
    """Can rsvld_conv3x3_halo_nhwc run this layer as RSVLD_F16Q8 (and would the halo kernel be chosen for it in the split precision)?
    -> the layer's L.ConvPlan (for ``_conv2d_q8``), or None."""
    ctx = _CTX.get()
    if not ctx.use_halo or act != L.ACT_NONE or pc.w.dtype != torch.float32:     # (_conv2d_q8 has no activation; _wq8 packs fp32 masters)
        return None
    plan, _ = _conv_plan(L.load(), _q8_conv_desc(B, H, W, Cc, pc, stride=stride, pad=pad, upsample=upsample, act=act, out_planes=out_planes))
    return plan if plan.halo_bn != 0 and plan.halo_wgs >= ctx.split_halo_min_wgs else None


def _q8_conv_desc(B, H, W, Cc, pc, *, stride=1, pad=1, upsample=False, act=L.ACT_NONE, out_planes=False, **operands):
    """The rsvld_conv_desc of ``pc`` on a ``[B, H, W, Cc]`` input as RSVLD_F16Q8 (``operands``: the tensors and scalars of ``_conv_desc``;
    absent tensors: null pointers).  ``_conv2d_q8`` launches it; ``_q8_conv_eligible`` asks the library's plan of it."""
    shape = (B, H, W, Cc)
    return _conv_desc(shape, 0, pc, _conv_geometry(shape, pc, stride, pad, upsample, act), L.F16Q8, int(not out_planes), stride=stride,
                      upsample=upsample, act=act, **operands)


def _conv2d_q8(xq, pc, *, rowvec, residual, alpha, beta, stats, plan):
    """3x3 / stride 1 / pad 1 on Q8Rows: fp32 out (+ fp32 residual), epilogue statistics for the next GroupNorm.  ``plan``: the layer's,
    from ``_q8_conv_eligible``."""
    B, H, W, Cc = xq.shape
    out = torch.empty((B, H, W, pc.cout_p), device=xq.t.device, dtype=torch.float32)
    d = _q8_conv_desc(B, H, W, Cc, pc, x=xq.t, w=_wq8(pc), rowvec=rowvec, residual=residual, out=out, alpha=alpha, beta=beta)
    flops = 2.0 * B * H * W * pc.cout * pc.cin * 9
    nbytes = 4.0 * (B * H * W * Cc + out.numel() + (0 if residual is None else residual.numel())) + 4.0 * pc.w.numel()
    _halo_launch(f"conv_halo_{plan.halo_bn}_q8" + _detail(B, H, W, Cc, 0, pc, 1, False), flops, nbytes, d, out, None, 0,
                 plan.halo_stat_tiles if stats else 0)
    out._nhwc = True
    return out


def _gn_ab_from_partials(x, x2, gamma, nbeta, groups, eps):
    """(scale, shift) fp32 ``[B, C1+C2, 2]`` of a GroupNorm over NHWC ``[x | x2]`` from the (sum, sumsq) partials their producers'
    epilogues attached (``_gn_part``: no pass over the tensors); None unless every source carries them."""
    part1 = getattr(x, "_gn_part", None)
    part2 = None if x2 is None else getattr(x2, "_gn_part", None)
    if part1 is None or (x2 is not None and part2 is None):
        return None
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    ab = torch.empty((B, C1 + C2, 2), device=x.device, dtype=torch.float32)
    _launch("groupnorm_ab_from_partials", 0.0, 0.0, lambda: L.check(L.load().rsvld_groupnorm_scale_shift_from_partials(
        _ptr(part1[0]), part1[1], C1, None if part2 is None else _ptr(part2[0]), 0 if part2 is None else part2[1],
        C2, _ptr(gamma), _ptr(nbeta), _ptr(ab), B, H * W, groups, eps, _stream()), "rsvld_groupnorm_scale_shift_from_partials"))
    return ab


def _gn_scale_shift_f32(x, x2, gamma, nbeta, groups, eps):
    """(scale, shift) fp32 ``[B, C1+C2, 2]`` of a GroupNorm over fp32 NHWC ``[x | x2]``: from the producers' epilogue partials when
    every source carries them (no pass over the tensors), else one statistics pass."""
    ab = _gn_ab_from_partials(x, x2, gamma, nbeta, groups, eps)
    if ab is not None:
        return ab
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    lib = L.load()
    ab = torch.empty((B, C1 + C2, 2), device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.rsvld_groupnorm_ws_bytes(B, H * W, C1 + C2, groups), device=x.device, dtype=torch.uint8)
    _launch("groupnorm_stats_split", 0.0, 4.0 * (x.numel() + (0 if x2 is None else x2.numel())), lambda: L.check(
        lib.rsvld_groupnorm_scale_shift_f32(_ptr(x), _ptr(x2), _ptr(gamma), _ptr(nbeta), _ptr(ab), B, H * W, C1, C2, groups, eps,
                                            _ptr(ws), _stream()), "rsvld_groupnorm_scale_shift_f32"))
    return ab


def _gn_apply_split(x, x2, ab, silu, planes, mod_scale1p=None, mod_shift=None, f16=False, q8=False):
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    Cc = C1 + C2
    mod_stride = _mod_stride(mod_scale1p)
    # (_mod_operands saw the tensors as the caller passed them: group_norm has since merged a Planes one into a contiguous fp32 tensor,
    #  which its plain partner -- a channel slice with another row stride, say -- must still agree with)
    if mod_scale1p is not None and (mod_shift.stride(-2) != mod_stride or mod_scale1p.stride(-1) != 1 or mod_shift.stride(-1) != 1
                                    or mod_scale1p.dtype != torch.float32 or mod_shift.dtype != torch.float32):
        raise L.RsvldError("group_norm: modulation tensors must be fp32, share a row stride and be channel-contiguous")
    f16 = f16 and planes          # the fp16 hand-over replaces a planes output only
    if q8:                        # RSVLD_F16Q8 rows (the input of a convolution with e4m3 cross terms)
        out = torch.empty((B, H, W, 2, Cc), device=x.device, dtype=torch.float16)
        _launch("groupnorm_apply_q8", 0.0, 8.0 * B * H * W * Cc, lambda: L.check(L.load().rsvld_groupnorm_apply_split(
            _ptr(x), _ptr(x2), _ptr(out), _ptr(ab), _ptr(mod_scale1p), _ptr(mod_shift), mod_stride, B, H * W, C1, C2, int(silu), 3, _stream()),
            "rsvld_groupnorm_apply_split"))
        return Q8Rows(out)
    if f16:
        out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float16)
    elif planes:
        out = torch.empty((B, H, W, 2, Cc), device=x.device, dtype=torch.bfloat16)
    else:
        out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float32)
    _launch("groupnorm_apply_split", 0.0, (6.0 if f16 else 8.0) * B * H * W * Cc, lambda: L.check(L.load().rsvld_groupnorm_apply_split(
        _ptr(x), _ptr(x2), _ptr(out), _ptr(ab), _ptr(mod_scale1p), _ptr(mod_shift), mod_stride, B, H * W, C1, C2, int(silu),
        2 if f16 else int(not planes), _stream()), "rsvld_groupnorm_apply_split"))
    if f16:
        return out
    if planes:
        return Planes(out)
    out._nhwc = True
    return out


def _detail(B, Ho, Wo, Cin, Cin2, pc, stride, upsample):
    if not _CTX.get().profile_detail:
        return ""
    return f" [{B}x{Ho}x{Wo} {Cin}+{Cin2}->{pc.cout_p} k{pc.kh} s{stride}{' up' if upsample else ''}]"


def _conv2d_split(x, pc, *, x2, stride, pad, upsample, rowvec, residual, act, alpha, beta, norm, stats, out_planes, out_group=None,
                  norm_group=None, group=None):
    """The split-operand product path of conv2d / linear: bf16 planes in (split here when the caller hands fp32), weight triples,
    the 16-bit kernels with dtype RSVLD_SPLIT; fp32 (or Planes, or -- a 1x1 layer whose consumer group takes fp16 -- fp16) out,
    fp32 residual."""

    if norm is not None:      # GroupNorm(+SiLU) over [x | x2]: its own apply pass writes ONE planes tensor (no concat, no fp32 copy)
        gamma, nbeta, groups, eps, silu = norm
        if isinstance(x, Planes) or isinstance(x2, Planes):
            raise L.RsvldError("conv2d (split): norm= needs the fp32 tensors")
        ab = _gn_scale_shift_f32(x, x2, gamma, nbeta, groups, eps)
        if f16_group(norm_group):     # the policy hands this convolution's input over in fp16: the weight-pair form (fp32 out, fp32 residual)
            x16 = _gn_apply_split(x, x2, ab, silu, planes=True, f16=True)
            return conv2d(x16, pc, stride=stride, pad=pad, upsample=upsample, rowvec=rowvec, residual=residual, act=act, alpha=alpha,
                          beta=beta, stats=stats, out_planes=out_planes, out_group=out_group, group=group)
        q8_plan = q8_group(norm_group) and _q8_conv_eligible(x.shape[0], x.shape[1], x.shape[2],
                                                             x.shape[3] + (0 if x2 is None else x2.shape[3]), pc, stride, pad, upsample, act,
                                                             out_planes)
        if q8_plan:
            # both operands keep ~22 bits, the two cross terms of the product run in e4m3 (RSVLD_F16Q8; SplitPolicy.q8_convs)
            return _conv2d_q8(_gn_apply_split(x, x2, ab, silu, planes=True, q8=True), pc, rowvec=rowvec, residual=residual, alpha=alpha,
                              beta=beta, stats=stats, plan=q8_plan)
        x, x2 = _gn_apply_split(x, x2, ab, silu, planes=True), None
    ctx = _CTX.get()
    x = to_planes(x)
    x2 = None if x2 is None else to_planes(x2)
    B, H, W, Cin = x.shape
    Cin2 = 0 if x2 is None else x2.shape[-1]
    geo = _conv_geometry(x.shape, pc, stride, pad, upsample, act)
    Ho, Wo, c_out = geo[2:]
    if residual is not None and out_planes:
        raise L.RsvldError("conv2d (split): a planes output takes no residual (the residual stream stays fp32)")
    # fp16 hand-over: a Linear / 1x1 layer (the implicit-GEMM kernels write it) whose consumer's layer group takes fp16 inputs
    out_f16 = bool(out_planes and f16_group(out_group) and pc.kh == 1 and pc.kw == 1 and stride == 1 and x2 is None and not upsample)
    if out_f16:
        out = torch.empty((B, Ho, Wo, c_out), device=x.device, dtype=torch.float16)
    elif out_planes:
        out = torch.empty((B, Ho, Wo, 2, c_out), device=x.device, dtype=torch.bfloat16)
    else:
        out = torch.empty((B, Ho, Wo, c_out), device=x.device, dtype=torch.float32)
    d = _conv_desc(x.shape, Cin2, pc, geo, L.SPLIT, 2 if out_f16 else int(not out_planes), stride=stride, upsample=upsample, act=act,
                   alpha=alpha, beta=beta, x=x.t, x2=None if x2 is None else x2.t, w=_w3(pc), rowvec=rowvec, residual=residual, out=out)
    lib = L.load()
    flops = 2.0 * B * Ho * Wo * pc.cout * pc.cin * pc.kh * pc.kw
    nbytes = 4.0 * (x.numel() + (0 if x2 is None else x2.numel()) + out.numel() / (2 if (out_planes or out_f16) else 1)
                    + (0 if residual is None else residual.numel())) + 6.0 * pc.w.numel()
    plan, rc = _conv_plan(lib, d)
    if ctx.use_halo and plan.halo_bn != 0 and plan.halo_wgs >= ctx.split_halo_min_wgs:
        _halo_launch(f"conv_halo_{plan.halo_bn}_split" + _detail(B, Ho, Wo, Cin, Cin2, pc, stride, upsample),
                     flops, nbytes, d, out, None, 0, plan.halo_stat_tiles if stats and not out_planes else 0)
    else:
        L.check(rc, "rsvld_plan_conv")
        _launch(("gemm_256x256_split" if plan.gemm256 else "conv_igemm_split") + _detail(B, Ho, Wo, Cin, Cin2, pc, stride, upsample),
                flops, nbytes, lambda: L.check(lib.rsvld_conv2d_nhwc(C.byref(d), _stream()), "rsvld_conv2d_nhwc"))
    if out_f16:
        return out
    if out_planes:
        return Planes(out)
    out._nhwc = True
    return out


def linear(x, pc, *, residual=None, act=L.ACT_NONE, alpha=1.0, beta=1.0, out_planes=False, out_group=None, group=None):
    """``[..., Cin] -> [..., Cout]`` on token-major tensors (a 1x1 conv over rows).  ``group``: the layer's weight group
    (``SplitPolicy.f16_weights``) where the consumer of its output does not name it."""
    # (contiguous rows: the reshapes below must be views -- a copy made here would hide a caller's layout mistake)
    if isinstance(x, Planes):
        _arg("linear", "x", x.t, torch.bfloat16)
    else:
        _arg("linear", "x", x, _ACT)
    if x.dim() < 1 or x.shape[-1] == 0:
        _bad("linear", "x", f"needs a channel dimension, got shape {tuple(x.shape)}")
    _arg("linear", "residual", residual, shape=tuple(x.shape[:-1]) + (None,), optional=True)
    shp = x.shape
    rows = x.numel() // shp[-1]
    res = None if residual is None else residual.reshape(1, 1, rows, residual.shape[-1])
    y = conv2d(x.reshape(1, 1, rows, shp[-1]), pc, pad=0, residual=res, act=act, alpha=alpha, beta=beta, out_planes=out_planes,
               out_group=out_group, group=group)
    return y.reshape(*shp[:-1], y.shape[-1])


# ----------------------------------------------------------------------------- norms
def _gn_operands(fn, x, x2, gamma, beta, stats=None, groups=None):
    """GroupNorm family: NHWC ``x`` (16-bit or fp32, contiguous), ``x2`` of its type and pixels, fp32 gamma / beta of C1 + C2
    channels, fp32 statistics ``[B, groups, 2]``."""
    _arg(fn, "x", x, _ACT, shape=(None,) * 4)
    _arg(fn, "x2", x2, x.dtype, shape=tuple(x.shape[:3]) + (None,), optional=True)
    Cc = x.shape[3] + (0 if x2 is None else x2.shape[3])
    _arg(fn, "gamma", gamma, torch.float32, shape=(Cc,), optional=True)
    _arg(fn, "beta", beta, torch.float32, shape=(Cc,), optional=True)
    if stats is not None or groups is not None:
        _arg(fn, "stats", stats, torch.float32, shape=(x.shape[0], groups, 2))


def _mod_operands(fn, x, x2, mod_scale1p, mod_shift, planes_ok=False):
    """ZeroSFT modulation: both or neither; of ``x``'s type and ``[B, H, W, C1 + C2]`` shape, channel slices of one stacked tensor
    (pixel-major rows of one stride, 16-byte aligned); planes where the split precision converts them."""
    if (mod_scale1p is None) != (mod_shift is None):
        _bad(fn, "mod_shift" if mod_shift is None else "mod_scale1p", "comes without its partner")
    if mod_scale1p is None:
        return
    B, H, W = x.shape[:3]
    Cc = x.shape[3] + (0 if x2 is None else x2.shape[3])
    for name, m in (("mod_scale1p", mod_scale1p), ("mod_shift", mod_shift)):
        if isinstance(m, Planes) and planes_ok:      # merged to a contiguous fp32 tensor first
            _arg(fn, name, m.t, torch.bfloat16, shape=(B, H, W, 2, Cc), layout=None)
            continue
        _arg(fn, name, m, x.dtype, shape=(B, H, W, Cc), layout="rows")
        ms = m.stride(2)
        if any(s != e for s, e, n in zip(m.stride(), (H * W * ms, W * ms, ms, 1), m.shape) if n > 1):
            _bad(fn, name, f"must be pixel-major rows of one stride, got strides {tuple(m.stride())}")
    if not isinstance(mod_scale1p, Planes) and not isinstance(mod_shift, Planes) and mod_scale1p.stride(2) != mod_shift.stride(2):
        _bad(fn, "mod_shift", "must share mod_scale1p's row stride")


def _mod_stride(mod_scale1p):
    """Row (pixel) stride in elements that both ZeroSFT modulation tensors share (``_mod_operands``); 0 without modulation."""
    return 0 if mod_scale1p is None else mod_scale1p.stride(-2)


def group_norm(x, gamma, beta, groups, eps, *, x2=None, silu=False, mod_scale1p=None, mod_shift=None, planes=False, group=None):
    """GroupNorm(+SiLU) over NHWC ``x`` (or the channel concat [x | x2]).  ``mod_scale1p`` / ``mod_shift``
    (ZeroSFT) may be channel slices of one stacked tensor: only their row stride must agree.
    ``planes=True`` (split precision only, ignored otherwise): the result only feeds a matrix product -> ``Planes``, or fp16 when
    the policy hands the inputs of that product's layer group ``group`` over in fp16."""
    _gn_operands("group_norm", x, x2, gamma, beta)
    _mod_operands("group_norm", x, x2, mod_scale1p, mod_shift, planes_ok=x.dtype == torch.float32 and _split_fast())
    if x.dtype == torch.float32 and _split_fast() and not isinstance(x, Planes):
        _need_gpu(x, x2, gamma, beta)
        ab = _gn_scale_shift_f32(x, x2, gamma, beta, groups, eps)
        return _gn_apply_split(x, x2, ab, silu, planes, as_f32(mod_scale1p) if mod_scale1p is not None else None,
                               as_f32(mod_shift) if mod_shift is not None else None, f16=f16_group(group))
    _need_gpu(x, x2, gamma, beta)
    if x.dtype == torch.float32:       # fp32 family: the two-source form concatenates first; statistics, then apply (+ modulation)
        if x2 is not None:
            x = concat_c(x, x2)
        return group_norm_apply(x, group_norm_stats(x, groups), gamma, beta, groups, eps, silu=silu,
                                mod_scale1p=mod_scale1p, mod_shift=mod_shift)
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    lib = L.load()
    ws = torch.empty(lib.rsvld_groupnorm_ws_bytes(B, H * W, C1 + C2, groups), device=x.device, dtype=torch.uint8)
    y = torch.empty((B, H, W, C1 + C2), device=x.device, dtype=x.dtype)
    nbytes = 3 * y.numel() * y.element_size()  # stats read + apply read + write
    _launch("groupnorm(3 kernels)", 0.0, nbytes, lambda: L.check(
        lib.rsvld_groupnorm_nhwc(_ptr(x), _ptr(x2), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(mod_scale1p),
                                 _ptr(mod_shift), _mod_stride(mod_scale1p), B, H * W, C1, C2, groups, eps, int(silu), _dt(x),
                                 _ptr(ws), _stream()), "rsvld_groupnorm_nhwc"))
    return y


def group_norm_stats(x, groups, *, x2=None):
    """-> fp32 ``[B, groups, 2]`` (mean, biased variance)."""
    _gn_operands("group_norm_stats", x, x2, None, None)
    _need_gpu(x, x2)
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    lib = L.load()
    if x.dtype == torch.float32 and _split_fast():
        if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
            raise L.RsvldError("group_norm_stats (split): contiguous fp32 NHWC tensors expected")
        ws = torch.empty(lib.rsvld_groupnorm_ws_bytes(B, H * W, C1 + C2, groups), device=x.device, dtype=torch.uint8)
        st = torch.empty((B, groups, 2), device=x.device, dtype=torch.float32)
        _launch("groupnorm_stats_split", 0.0, 4.0 * (x.numel() + (0 if x2 is None else x2.numel())), lambda: L.check(
            lib.rsvld_groupnorm_stats_f32_fast(_ptr(x), _ptr(x2), _ptr(st), B, H * W, C1, C2, groups, _ptr(ws), _stream()),
            "rsvld_groupnorm_stats_f32_fast"))
        return st
    if x.dtype == torch.float32:
        if x2 is not None or not x.is_contiguous():
            raise L.RsvldError("group_norm_stats (fp32): one contiguous NHWC tensor expected")
        ws = torch.empty(lib.rsvld_groupnorm_f32_ws_bytes(B, H * W, C1, groups), device=x.device, dtype=torch.uint8)
        st = torch.empty((B, groups, 2), device=x.device, dtype=torch.float32)
        _launch("groupnorm_stats_f32", 0.0, 4.0 * x.numel(), lambda: L.check(
            lib.rsvld_groupnorm_stats_f32(_ptr(x), _ptr(st), B, H * W, C1, groups, _ptr(ws), _stream()), "rsvld_groupnorm_stats_f32"))
        return st
    ws = torch.empty(lib.rsvld_groupnorm_ws_bytes(B, H * W, C1 + C2, groups), device=x.device, dtype=torch.uint8)
    st = torch.empty((B, groups, 2), device=x.device, dtype=torch.float32)
    L.check(lib.rsvld_groupnorm_stats(_ptr(x), _ptr(x2), _ptr(st), B, H * W, C1, C2, groups, _dt(x), _ptr(ws),
                                      _stream()), "rsvld_groupnorm_stats")
    return st


def group_norm_apply(x, stats, gamma, beta, groups, eps, *, x2=None, silu=False, mod_scale1p=None, mod_shift=None, planes=False):
    """``mod_*`` (ZeroSFT modulation) with supplied statistics exists in the fp32 family only.
    ``planes=True`` (split precision only): the result only feeds a matrix product -> ``Planes``."""
    _gn_operands("group_norm_apply", x, x2, gamma, beta, stats=stats, groups=groups)
    _mod_operands("group_norm_apply", x, x2, mod_scale1p, mod_shift)
    _need_gpu(x, x2, stats, gamma, beta)
    if x.dtype == torch.float32 and _split_fast() and not isinstance(x, Planes):
        B, H, W, C1 = x.shape
        Cc = C1 + (0 if x2 is None else x2.shape[-1])
        ab = torch.empty((B, Cc, 2), device=x.device, dtype=torch.float32)
        L.check(L.load().rsvld_groupnorm_scale_shift_from_stats(_ptr(stats), _ptr(gamma), _ptr(beta), _ptr(ab), B, Cc, groups, eps,
                                                                _stream()), "rsvld_groupnorm_scale_shift_from_stats")
        return _gn_apply_split(x, x2, ab, silu, planes, mod_scale1p, mod_shift)
    if mod_scale1p is not None and x.dtype != torch.float32:
        raise L.RsvldError("group_norm_apply: modulation with supplied statistics is an fp32-family feature (use group_norm)")
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    y = torch.empty((B, H, W, C1 + C2), device=x.device, dtype=x.dtype)
    if x.dtype == torch.float32:
        if x2 is not None or not x.is_contiguous():
            raise L.RsvldError("group_norm_apply (fp32): one contiguous NHWC tensor expected")
        _launch("groupnorm_apply_f32", 0.0, 8.0 * x.numel(), lambda: L.check(L.load().rsvld_groupnorm_apply_f32(
            _ptr(x), _ptr(y), _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(mod_scale1p), _ptr(mod_shift), _mod_stride(mod_scale1p),
            B, H * W, C1, groups, eps, int(silu), _stream()), "rsvld_groupnorm_apply_f32"))
        y._nhwc = True
        return y
    L.check(L.load().rsvld_groupnorm_apply(_ptr(x), _ptr(x2), _ptr(y), _ptr(stats), _ptr(gamma), _ptr(beta), None,
                                           None, 0, B, H * W, C1, C2, groups, eps, int(silu), _dt(x), _stream()),
            "rsvld_groupnorm_apply")
    return y


def layer_norm(x, gamma, beta, eps=1e-5, planes=False, group=None):
    """``planes=True`` (split precision only, ignored otherwise): the result only feeds matrix products -> ``Planes``, or fp16 when
    the policy hands the inputs of those products' layer group ``group`` over in fp16."""
    _arg("layer_norm", "x", x, _ACT)
    if x.dim() < 1 or x.numel() == 0:
        _bad("layer_norm", "x", f"needs rows of channels, got shape {tuple(x.shape)}")
    Cc = x.shape[-1]
    _arg("layer_norm", "gamma", gamma, torch.float32, shape=(Cc,), optional=True)
    _arg("layer_norm", "beta", beta, torch.float32, shape=(Cc,), optional=True)
    _need_gpu(x, gamma, beta)
    rows = x.numel() // Cc
    if x.dtype == torch.float32 and _split_fast():
        if not x.is_contiguous():
            raise L.RsvldError("layer_norm (split): contiguous rows expected")
        f16 = planes and f16_group(group)
        if f16:
            y = torch.empty(x.shape, device=x.device, dtype=torch.float16)
        elif planes:
            y = torch.empty(tuple(x.shape[:-1]) + (2, Cc), device=x.device, dtype=torch.bfloat16)
        else:
            y = torch.empty_like(x)
        _launch("layernorm_split", 0.0, (6.0 if f16 else 8.0) * x.numel(), lambda: L.check(L.load().rsvld_layernorm_split(
            _ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), rows, Cc, eps, 2 if f16 else int(not planes), _stream()), "rsvld_layernorm_split"))
        return y if f16 else (Planes(y) if planes else y)
    y = torch.empty_like(x)
    if x.dtype == torch.float32:
        if not x.is_contiguous():
            raise L.RsvldError("layer_norm (fp32): contiguous rows expected")
        _launch("layernorm_f32", 0.0, 8.0 * x.numel(), lambda: L.check(L.load().rsvld_layernorm_f32(
            _ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), rows, Cc, eps, _stream()), "rsvld_layernorm_f32"))
        return y
    L.check(L.load().rsvld_layernorm(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), rows, Cc, eps, _dt(x), _stream()),
            "rsvld_layernorm")
    return y


# ----------------------------------------------------------------------------- attention
def attention(q, k, v, heads, scale=None):
    """q ``[B, Nq, heads*D]``, k/v ``[B, Nk, heads*D]`` (views with a token stride are fine, e.g.
    slices of a fused qkv tensor) -> ``[B, Nq, heads*D]`` contiguous.
    In the split precision the policy decides (``SplitPolicy.f16_inputs``): with "attn" the operands are fp16 (handed over as fp16 by
    their producers, or converted here) and the 16-bit kernels run; the result is fp16 when "attn_out" is set (its consumer then runs
    as fp16 x weight pairs) and planes otherwise.  Without "attn" (the VAE's policy: its single-head attentions are a rounding error
    of the image's time and a third of the mode's Stage-2 distance from the reference when run in fp16, 4.4e-4 -> 3.0e-4 max after
    50 steps) the fused split kernels run on planes."""
    split = any(isinstance(t, Planes) for t in (q, k, v)) or (q.dtype == torch.float32 and _split_fast())
    for name, t in (("q", q), ("k", k), ("v", v)):
        if isinstance(t, Planes):
            _arg("attention", name, t.t, torch.bfloat16, shape=(None, None, 2, None), layout=None)
        else:   # token-stride views (slices of a fused q | k | v) are read in place: rows, not contiguity
            _arg("attention", name, t, (torch.float32, torch.float16) if split else (_ACT if t is q else q.dtype), shape=(None,) * 3,
                 layout="rows")
    if heads <= 0 or q.shape[2] % heads:
        _bad("attention", "q", f"has {q.shape[2]} channels, not a multiple of heads = {heads}")
    for name, t in (("k", k), ("v", v)):
        if tuple(t.shape) != (q.shape[0], k.shape[1], q.shape[2]):
            _bad("attention", name, f"has shape {tuple(t.shape)}, expected [B, Nk, H*D] = {(q.shape[0], k.shape[1], q.shape[2])}")
    if split:
        return _attention_split(q, k, v, heads, scale)
    _need_gpu(q, k, v)
    B, Nq, HD = q.shape
    Nk = k.shape[1]
    D = HD // heads
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    (qb, qt, q1), (kb, kt, k1), (vb, vt, v1) = q.stride(), k.stride(), v.stride()    # read once: checks, plan and launch
    if q1 != 1 or k1 != 1 or v1 != 1:
        raise L.RsvldError("attention: last dim must be contiguous")
    out = torch.empty((B, Nq, HD), device=q.device, dtype=q.dtype)
    ob, ot, _ = out.stride()
    lib = L.load()
    flops = 4.0 * B * heads * Nq * Nk * D
    nbytes = (q.shape[0] * Nq * HD * 2 + 2 * B * Nk * HD) * q.element_size()
    if q.dtype == torch.float32:
        if k.dtype != torch.float32 or v.dtype != torch.float32:
            raise L.RsvldError("attention (fp32): q, k, v must all be fp32")
        fn = lib.rsvld_attention_f32_split if _policy() is not None else lib.rsvld_attention_f32
        _launch(f"attention_f32{'_split' if _policy() is not None else ''}_d{D}", flops, nbytes, lambda: L.check(
            fn(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, heads, Nq, Nk, D, qb, qt, kb, kt, vb, vt, ob, ot, scale, _stream()),
            "rsvld_attention_f32"))
        return out
    ctx = _CTX.get()
    tune = ctx.d64_kernel if D == 64 else ctx.d512_kernel
    # The library's plan of this launch, asked once: the split-KV partials (D = 512, small grids) are the caller's allocation; a
    # refused plan asks for no workspace, and the launch below reports the refusal.  Keys and values that are ONE tensor (same
    # pointer and strides) get the shared-tile kernels.
    pk, pv = k.data_ptr(), v.data_ptr()
    plan = L.AttentionPlan()                    # (ctypes passes the structure by reference)
    lib.rsvld_plan_attention(B, heads, Nq, Nk, D, ctx.plan_div, tune, pk == pv and kb == vb and kt == vt, kt, vt, plan)
    ws_bytes = plan.ws_bytes
    ws = torch.empty(ws_bytes, device=q.device, dtype=torch.uint8) if ws_bytes > 0 else None
    # (profiler group: the short cross-attention launches -- 77 text keys -- are a different kernel and a different regime than
    #  the self-attention of the same layer: kept apart so that the roofline of the dominant group describes ONE kind of launch)
    _launch(f"attention_d{D}" + ("_cross" if (D == 64 and Nk != Nq) else ""), flops, nbytes, lambda: L.check(
        lib.rsvld_attention_tuned(_ptr(q), C.c_void_p(pk), C.c_void_p(pv), _ptr(out), B, heads, Nq, Nk, D, qb, qt, kb, kt, vb, vt,
                                  ob, ot, scale, _dt(q), ctx.plan_div, _ptr(ws), _stream(), tune),
        "rsvld_attention"))
    if _split_fast() and not f16_group("attn_out"):   # a split-precision network whose to_out wants planes (exact: 11 bits fit hi + lo)
        return _f16_to_planes(out)
    return out


def _split_gemm(xt, w3, out, M, K, N, out_f32, name):
    """``out[M, N] = x[M, K] w[N, K]^T`` in the split precision: ``xt`` contiguous planes ``[M, 2, K]``, ``w3`` triples ``[N, 3K]``,
    ``out`` fp32 ``[M, N]`` or planes ``[M, 2, N]`` (rsvld_conv2d_nhwc as a 1x1 layer; plans on the whole call)."""
    d = _conv_desc((1, 1, M, K), 0, PackedConv(w3, None, K, N, K, N, 1, 1), (0, 0, 1, M, N), L.SPLIT, int(out_f32), x=xt, w=w3, out=out,
                   plan_div=1)
    _launch(name, 2.0 * M * K * N, 4.0 * M * K + 6.0 * N * K + 4.0 * M * N,
            lambda: L.check(L.load().rsvld_conv2d_nhwc(C.byref(d), _stream()), "rsvld_conv2d_nhwc"))


def _planes_to_f16(x):
    """Planes / fp32 ``[B, N, C]`` (channel slices of a fused planes tensor are read in place) -> contiguous fp16 ``[B, N, C]``."""
    if not isinstance(x, Planes):
        return x.to(torch.float16)
    t = x.t                                             # [B, N, 2, C]
    B, N, _, C = t.shape
    if t.stride(3) != 1 or t.stride(0) != N * t.stride(1):
        t = t.contiguous()
    out = torch.empty((B, N, C), device=t.device, dtype=torch.float16)
    _launch("planes_to_f16", 0.0, 6.0 * B * N * C, lambda: L.check(L.load().rsvld_planes_to_f16(
        _ptr(t), t.stride(1), t.stride(2), _ptr(out), C, B * N, C, _stream()), "rsvld_planes_to_f16"))
    return out


def _f16_to_planes(x):
    """contiguous fp16 ``[..., C]`` -> Planes (exact)."""
    C = x.shape[-1]
    t = torch.empty(tuple(x.shape[:-1]) + (2, C), device=x.device, dtype=torch.bfloat16)
    _launch("f16_to_planes", 0.0, 6.0 * x.numel(), lambda: L.check(L.load().rsvld_f16_to_planes(
        _ptr(x), C, _ptr(t), x.numel() // C, C, _stream()), "rsvld_f16_to_planes"))
    return Planes(t)


def _attention_split(q, k, v, heads, scale):
    """Planes / fp32 operands in a split-precision network.  Policy "attn": the operands leave the planes as fp16 and the 16-BIT attention
    kernels run (attn_d64c / attn_d512b at 1 100-1 240 TFLOP/s instead of the three-MFMA kernels at 400-440 effective; measured against
    the reference's CPU runs after 50 + 50 steps, rounding ONLY q, k, v, P costs 4e-5 in Stage 1 and 2.5e-4 in Stage 2, where rounding
    the weights costs 2e-3 and every activation 3e-3: DESIGN.md).  Otherwise: the fused split attention kernels."""
    if f16_group("attn") and q.shape[-1] % 8 == 0:
        shared = k is v
        q16, k16 = _planes_to_f16(q), _planes_to_f16(k)
        v16 = k16 if shared else _planes_to_f16(v)
        return attention(q16, k16, v16, heads, scale)     # (-> fp16 or planes, by "attn_out")
    return _attention_split_kernels(q, k, v, heads, scale)


def _attention_split_kernels(q, k, v, heads, scale):
    """Attention in the split precision -> ``Planes [B, Nq, heads*D]`` (its consumer is always a projection).
    D = 64: the fused flash kernel on planes (rsvld_attention_split_d64).  Other head sizes (single-head d = 512 of SR3 and the
    VAE): two split GEMMs around a row softmax per block of query rows -- S = Q K^T (fp32) -> P = softmax(scale S) (planes) ->
    O = P V -- with K and V re-packed once as the GEMMs' weight triples."""
    shared = k is v
    def prep(t):
        if isinstance(t, Planes):
            return t
        return to_planes(t.contiguous())
    q = prep(q)
    k = prep(k)
    v = k if shared else prep(v)
    _need_gpu(q.t, k.t, v.t)
    B, Nq, HD = q.shape
    Nk = k.shape[1]
    D = HD // heads
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    lib = L.load()
    out = torch.empty((B, Nq, 2, HD), device=q.t.device, dtype=torch.bfloat16)
    flops = 4.0 * B * heads * Nq * Nk * D
    if D == 64:
        for t in (q.t, k.t, v.t):
            if t.stride(3) != 1:
                raise L.RsvldError("attention (split): last dim must be contiguous")
        nbytes = 4.0 * (2 * B * Nq * HD + 2 * B * Nk * HD)
        _launch("attention_split_d64" + ("_cross" if Nk != Nq else ""), flops, nbytes, lambda: L.check(lib.rsvld_attention_split_d64(
            _ptr(q.t), _ptr(k.t), _ptr(v.t), _ptr(out), B, heads, Nq, Nk,
            q.t.stride(0), q.t.stride(1), q.t.stride(2), k.t.stride(0), k.t.stride(1), k.t.stride(2),
            v.t.stride(0), v.t.stride(1), v.t.stride(2), out.stride(0), out.stride(1), out.stride(2), scale, 0, _stream()),
            "rsvld_attention_split_d64"))
        return Planes(out)
    if D == 512 and heads == 1 and shared and Nq >= _CTX.get().split_d512_fused_min:
        # keys and values are ONE planes tensor (SR3's re-associated SelfAttention): the fused kernel, two waves per 32 query rows
        nbytes = 4.0 * (2 * B * Nq * HD + B * Nk * HD)
        _launch("attention_split_d512", flops, nbytes, lambda: L.check(lib.rsvld_attention_split_d512_shared(
            _ptr(q.t), _ptr(k.t), _ptr(out), B, Nq, Nk, q.t.stride(0), q.t.stride(1), q.t.stride(2),
            k.t.stride(0), k.t.stride(1), k.t.stride(2), out.stride(0), out.stride(1), out.stride(2), scale, 0, _stream()),
            "rsvld_attention_split_d512_shared"))
        return Planes(out)
    if D % 8:
        raise L.RsvldError("attention (split): head dim must be a multiple of 8")
    Nk_p = (Nk + 7) // 8 * 8
    rows_blk = max(256, min(Nq, (_CTX.get().split_attn_s_bytes // (4 * Nk_p)) // 256 * 256))
    dev = q.t.device
    for b in range(B):
        for h in range(heads):
            def head(t):      # contiguous planes [N, 2, D] of (b, h)
                th = t[b, :, :, h * D:(h + 1) * D]
                return th if th.is_contiguous() else th.contiguous()
            qh, kh = head(q.t), head(k.t)
            vh = kh if shared else head(v.t)
            w1 = torch.empty((Nk_p, 3 * D), device=dev, dtype=torch.bfloat16)
            L.check(lib.rsvld_planes_to_triple(_ptr(kh), _ptr(w1), Nk, Nk_p, D, 2 * D, _stream()), "rsvld_planes_to_triple")
            w2 = torch.empty((D, 3 * Nk_p), device=dev, dtype=torch.bfloat16)
            L.check(lib.rsvld_planes_transpose_triple(_ptr(vh), _ptr(w2), Nk, Nk_p, D, 2 * D, _stream()), "rsvld_planes_transpose_triple")
            oh = out[b] if heads == 1 else torch.empty((Nq, 2, D), device=dev, dtype=torch.bfloat16)
            for r0 in range(0, Nq, rows_blk):
                m = min(rows_blk, Nq - r0)
                s_blk = torch.empty((m, Nk_p), device=dev, dtype=torch.float32)
                _split_gemm(qh[r0:r0 + m], w1, s_blk, m, D, Nk_p, True, f"attention_split_gemm_qk_d{D}")
                p_blk = torch.empty((m, 2, Nk_p), device=dev, dtype=torch.bfloat16)
                _launch("attention_split_softmax", 0.0, 12.0 * m * Nk_p, lambda: L.check(lib.rsvld_softmax_rows_split(
                    _ptr(s_blk), _ptr(p_blk), m, Nk, Nk_p, Nk_p, scale, _stream()), "rsvld_softmax_rows_split"))
                del s_blk
                _split_gemm(p_blk, w2, oh[r0:r0 + m], m, Nk_p, D, False, f"attention_split_gemm_pv_d{D}")
                del p_blk
            if heads != 1:
                out[b, :, :, h * D:(h + 1) * D] = oh
    return Planes(out)


# The decode-step operators: ONE implementation each for ``B`` activation rows / sequences (``rsvld_amd.decode_rows`` is their public
# ``[B, .]`` face, ``w8`` holds the e4m3 product); the single-row functions below are the ``B = 1`` case on the caller's storage.
MAX_ROWS = 8      # RSVLD_DECODE_MAX_ROWS


def _rows(fn, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        _bad(fn, "x", f"must be a [B, K] tensor of activation rows, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    B = x.shape[0]
    if not 1 <= B <= MAX_ROWS:
        _bad(fn, "x", f"has {B} rows, expected 1..{MAX_ROWS}")
    return B


GEMV_KERNELS = ("valu", "mfma")    # the two families of decode products: csrc/gemv.hip / csrc/gemv_mma.hip


def _gemv_rows(fn, launch, w, scale, x, bias, norm, residual, glu, *, w8, single, kernel="valu"):
    """``fn`` (the public name errors carry; ``launch``: the profiler's) on ``B`` rows: ``w [N, K]`` 16-bit, or (``w8``) e4m3 bytes with
    ``scale [N]``.  A single-row function reaches the library through its own entry point, which is the ``B = 1`` call of the rows one.
    ``kernel="mfma"`` (rows functions only): the same operands, checks and errors, launched through the MFMA entry points -- at every
    ``B``, one row included."""
    if kernel not in GEMV_KERNELS or (single and kernel != "valu"):
        raise ValueError(f"{fn}: kernel={kernel!r}, expected one of {GEMV_KERNELS if not single else GEMV_KERNELS[:1]}")
    _arg(fn, "q" if w8 else "w", w, torch.uint8 if w8 else _HALF, shape=(None, None))
    N, K = w.shape
    if w8 and (N == 0 or K == 0 or K % 16):
        _bad(fn, "q", f"has shape {tuple(w.shape)}: rows of whole 16-byte pieces of e4m3 (K % 16 == 0) expected")
    B = 1 if single else _rows(fn, x)
    nw, eps = (None, 0.0) if norm is None else norm
    Kx = 2 * K if glu else K
    if w8:
        _arg(fn, "scale", scale, torch.float32, numel=N)
    # a per-row operand: [B, n]; a single-row function takes its row in any shape of n elements and returns [N]
    if single:
        dt = _arg(fn, "x", x, _HALF if w8 else w.dtype, numel=Kx).dtype
    else:
        dt = _arg(fn, "x", x, _HALF if w8 else w.dtype, shape=(B, Kx)).dtype
    _arg(fn, "bias", bias, dt, numel=N, optional=True)
    _arg(fn, "norm weight", nw, dt, numel=Kx, optional=True)
    if single:
        _arg(fn, "residual", residual, dt, numel=N, optional=True)
    else:
        _arg(fn, "residual", residual, dt, shape=(B, N), optional=True)
    if glu and nw is not None:
        _bad(fn, "norm weight", "cannot be combined with glu")
    _need_gpu(w, scale, x, bias, nw, residual)
    y = torch.empty(N if single else (B, N), device=x.device, dtype=dt)
    entry = _GEMV_ENTRY[w8, single] if kernel == "valu" else _GEMV_MMA_ENTRY[w8]
    args = (_ptr(x), _ptr(bias), _ptr(nw), float(eps), _ptr(residual), int(glu), _ptr(y), N, K)
    args = ((_ptr(w), _ptr(scale)) if w8 else (_ptr(w),)) + args + ((_dt(x), _stream()) if single else (B, _dt(x), _stream()))
    call = getattr(L.load(), entry)
    _launch(launch, 2.0 * B * N * K, N * K + N * 4 + B * (K + N) * 2 if w8 else (N * K + B * (K + N)) * 2, lambda: L.check(call(*args), entry))
    return y


_GEMV_ENTRY = {(False, True): "rsvld_gemv_fused", (False, False): "rsvld_gemv_rows_fused",
               (True, True): "rsvld_gemv_w8_fused", (True, False): "rsvld_gemv_w8_rows_fused"}
_GEMV_MMA_ENTRY = {False: "rsvld_gemv_mma_rows_fused", True: "rsvld_gemv_w8_mma_rows_fused"}


def gemv(w, x, bias=None):
    """``w [N, K]`` (16-bit, rows contiguous) times ONE activation row ``x [K]`` (+ ``bias [N]``) -> ``[N]``: the weight-streaming
    products of the caption pass's token loop (HBM-bound, no tile, no MFMA): ``gemv_fused`` with nothing folded in."""
    return _gemv_rows("gemv", "gemv", w, None, x, bias, None, None, False, w8=False, single=True)


def gemv_fused(w, x, bias=None, *, norm=None, residual=None, glu=False):
    """``gemv`` with the element-wise neighbours of a Llama decode step folded in (rsvld_gemv_fused): ``norm=(weight, eps)``: the product runs
    on RMSNorm(x) * weight; ``glu``: x holds ``[gate | up]`` (2 K elements) and the product runs on silu(gate) * up; ``residual [N]``: the
    result is residual + (w x + bias).  ``decode_rows.gemv_rows`` on one row."""
    return _gemv_rows("gemv_fused", "gemv", w, None, x, bias, norm, residual, glu, w8=False, single=True)


DECODE_ATTENTION_KERNELS = ("valu", "mfma")    # the two decode-step attentions of csrc/decode_attention.hip: da_kernel / dam_kernel


def _decode_attention_rows(fn, qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws, single, kernel="valu"):
    """``fn`` on ``B`` sequences with caches ``[B, n_kv, max_len, 128]``; ``single``: caches ``[n_kv, max_len, 128]``, one sequence.
    ``kernel="mfma"``: the same operands, checks and errors, launched through rsvld_llama_decode_attention_mma_rows (one sequence is its
    ``B = 1`` call) under the launch name ``llama_decode_attention_mma_rows``, with that entry's own workspace size."""
    if kernel not in DECODE_ATTENTION_KERNELS:
        raise ValueError(f"{fn}: kernel={kernel!r}, expected one of {DECODE_ATTENTION_KERNELS}")
    mma = kernel == "mfma"
    _arg(fn, "kcache", kcache, _HALF, shape=(n_kv, None, None) if single else (None, n_kv, None, None))
    hd, max_len = kcache.shape[-1], kcache.shape[-2]
    B = 1 if single else kcache.shape[0]
    if not 1 <= B <= MAX_ROWS:
        _bad(fn, "kcache", f"holds {B} sequences, expected 1..{MAX_ROWS}")
    _arg(fn, "vcache", vcache, kcache.dtype, shape=tuple(kcache.shape))
    for name, t, n in (("qkv", qkv, (n_q + 2 * n_kv) * hd), ("cos", cos, hd), ("sin", sin, hd)):     # (per sequence, as in _gemv_rows)
        if single:
            _arg(fn, name, t, kcache.dtype, numel=n)
        else:
            _arg(fn, name, t, kcache.dtype, shape=(B, n))
    if single:
        _arg(fn, "pos", pos, torch.int64, numel=1)
    else:
        _arg(fn, "pos", pos, torch.int64, shape=(B,))
    _arg(fn, "ws", ws, torch.float32, shape=(None,), optional=True)
    _need_gpu(qkv, cos, sin, pos, kcache, vcache, ws)
    from .decode_rows import decode_attention_ws_floats   # (that module imports this one)
    lib = L.load()
    ws_n = decode_attention_ws_floats(n_q, n_kv, max_len, B, kernel)
    if ws is None:
        ws = torch.empty(ws_n, device=qkv.device, dtype=torch.float32)
    elif ws.numel() < ws_n:
        _bad(fn, "ws", f"has {ws.numel()} fp32 elements, the step needs {ws_n}")
    out = torch.empty(n_q * hd if single else (B, n_q * hd), device=qkv.device, dtype=qkv.dtype)
    entry = "rsvld_llama_decode_attention_mma_rows" if mma else "rsvld_llama_decode_attention" if single else "rsvld_llama_decode_attention_rows"
    args = (_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(kcache), _ptr(vcache), _ptr(out), _ptr(ws), n_q, n_kv, hd, max_len)
    args += (float(scale), _dt(qkv), _stream()) if single and not mma else (B, float(scale), _dt(qkv), _stream())
    call = getattr(lib, entry)
    _launch("llama_decode_attention_mma_rows" if mma else fn, 0.0, 0.0, lambda: L.check(call(*args), entry))
    return out


def llama_decode_attention(qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws=None, kernel="valu"):
    """One decode step of grouped-query attention over a static cache (rsvld_llama_decode_attention): ``qkv`` = the new token's q | k | v rows,
    ``pos`` a DEVICE int64 scalar; the caches ``[n_kv, max_len, 128]`` are updated at ``pos``; ``ws`` (optional, re-usable): an fp32
    tensor of rsvld_llama_decode_attention_ws_bytes (scratch: no initial state).  A position outside ``[0, max_len)`` is clamped by the kernel.
    -> ``[n_q * 128]``.  ``decode_rows.llama_decode_attention_rows`` on one sequence; ``kernel``: as there."""
    return _decode_attention_rows("llama_decode_attention", qkv, cos, sin, pos, kcache, vcache, n_q, n_kv, scale, ws, True, kernel)


def _prefill_attention(fn, q, kcache, vcache, n_q, n_kv, scale, pos0):
    """``prefill_attention.llama_prefill_attention`` (its public face): operand contracts, the output, the launch."""
    _arg(fn, "kcache", kcache, _HALF, shape=(n_kv, None, None))
    max_len, hd = kcache.shape[1], kcache.shape[2]
    _arg(fn, "vcache", vcache, kcache.dtype, shape=tuple(kcache.shape))
    if not isinstance(q, torch.Tensor) or q.dim() not in (2, 3):
        _bad(fn, "q", f"must be a [T, n_q * {hd}] or [T, n_q, {hd}] tensor, got {tuple(q.shape) if isinstance(q, torch.Tensor) else type(q).__name__}")
    T = q.shape[0]
    _arg(fn, "q", q, kcache.dtype, shape=(T, n_q * hd) if q.dim() == 2 else (T, n_q, hd), layout="rows")
    if q.dim() == 3 and n_q > 1 and q.stride(1) != hd:
        _bad(fn, "q", f"must hold a token's heads side by side, got strides {tuple(q.stride())}")
    q_ts = q.stride(0) if T > 1 else n_q * hd
    if not isinstance(pos0, int) or isinstance(pos0, bool):
        _bad(fn, "pos0", f"must be a host int (the prefill is not graph-captured), got {type(pos0).__name__}")
    if T < 1 or pos0 < 0 or pos0 + T > max_len:
        _bad(fn, "q", f"holds {T} positions from {pos0} on, the cache holds {max_len}")
    if q_ts < n_q * hd:
        _bad(fn, "q", f"has overlapping token rows (strides {tuple(q.stride())})")
    if n_kv < 1 or n_q % n_kv:
        _bad(fn, "q", f"has {n_q} heads on {n_kv} kv heads")
    _need_gpu(q, kcache, vcache)
    out = torch.empty((T, n_q * hd), device=q.device, dtype=q.dtype)
    lib = L.load()
    # causal: 2 (QK^T, PV) x 2 T (pos0 + (T + 1) / 2) n_q hd FLOP; q and out once, the filled prefix of both caches once per row block
    flops = 4.0 * n_q * hd * T * (pos0 + (T + 1) / 2.0)
    nbytes = (2 * T * n_q * hd + 2 * n_kv * (pos0 + T) * hd) * 2
    _launch(fn, flops, nbytes, lambda: L.check(
        lib.rsvld_llama_prefill_attention(_ptr(q), q_ts, _ptr(kcache), _ptr(vcache), _ptr(out), T, pos0, n_q, n_kv, hd, max_len, float(scale),
                                          _dt(q), _stream()), "rsvld_llama_prefill_attention"))
    return out


# ----------------------------------------------------------------------------- small fp32 layers
def linear_small(x, w, b, act_in=0, act_out=0):
    """fp32 ``[rows, in] -> [rows, out]`` with torch nn.Linear weight layout."""
    _arg("linear_small", "x", x, torch.float32, shape=(None, None))
    rows, in_f = x.shape
    _arg("linear_small", "w", w, torch.float32, shape=(None, in_f))
    out_f = w.shape[0]
    _arg("linear_small", "b", b, torch.float32, shape=(out_f,), optional=True)
    _need_gpu(x, w, b)
    y = torch.empty((rows, out_f), device=x.device, dtype=torch.float32)
    L.check(L.load().rsvld_linear_small_f32(_ptr(x), _ptr(w), _ptr(b), _ptr(y), rows, in_f, out_f, act_in, act_out,
                                            _stream()), "rsvld_linear_small_f32")
    return y


def sinusoidal(t, dim, kind):
    # (any real ``t`` of any layout: converted to a contiguous fp32 copy below)
    if not isinstance(t, torch.Tensor) or t.dtype == torch.bool or t.is_complex():
        _bad("sinusoidal", "t", f"must be a real tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    _need_gpu(t)
    t = t.reshape(-1).contiguous().float()
    out = torch.empty((t.numel(), dim), device=t.device, dtype=torch.float32)
    L.check(L.load().rsvld_sinusoidal_embedding(_ptr(t), _ptr(out), t.numel(), dim, kind, _stream()),
            "rsvld_sinusoidal_embedding")
    return out


# ----------------------------------------------------------------------------- layout / elementwise
def nchw_to_nhwc(src, dtype, c_dst=None, c_off=0, out=None, scale=1.0):
    """fp32 NCHW (* scale) -> 16-bit (or fp32) NHWC with channels padded to ``c_dst`` (default: next multiple of 8)."""
    # (``src`` of any floating type and layout: converted to a contiguous fp32 copy below)
    _arg("nchw_to_nhwc", "src", src, (torch.float32, torch.float16, torch.bfloat16, torch.float64), shape=(None,) * 4, layout=None)
    B, Cc, H, W = src.shape
    if out is not None:
        _arg("nchw_to_nhwc", "out", out, _ACT, shape=(B, H, W, None))
        if c_off < 0 or c_off + Cc > out.shape[-1]:
            _bad("nchw_to_nhwc", "out", f"has {out.shape[-1]} channels, the window [{c_off}, {c_off + Cc}) does not fit")
    elif dtype not in _ACT:
        _bad("nchw_to_nhwc", "dtype", f"is {dtype}, expected one of {_ACT}")
    elif c_off < 0 or c_off + Cc > (pad8(Cc) if c_dst is None else c_dst):
        _bad("nchw_to_nhwc", "src", f"has {Cc} channels: they do not fit [{c_off}, c_dst = {c_dst})")
    _need_gpu(src, out)
    src = src.contiguous().float()
    if out is None:
        c_dst = pad8(Cc) if c_dst is None else c_dst
        out = torch.empty((B, H, W, c_dst), device=src.device, dtype=dtype)
        zero = 1
    else:
        c_dst, zero = out.shape[-1], 0
    if out.dtype == torch.float32:
        L.check(L.load().rsvld_nchw_f32_to_nhwc_f32(_ptr(src), _ptr(out), B, Cc, H, W, c_dst, c_off, zero, scale, _stream()),
                "rsvld_nchw_f32_to_nhwc_f32")
        out._nhwc = True     # an fp32 4-d tensor is otherwise taken for NCHW by the VAE's input adapter
        return out
    L.check(L.load().rsvld_nchw_f32_to_nhwc(_ptr(src), _ptr(out), B, Cc, H, W, c_dst, c_off, zero, scale, _DT[out.dtype],
                                            _stream()), "rsvld_nchw_f32_to_nhwc")
    return out


def nhwc_to_nchw(src, channels=None, c_off=0):
    """NHWC (16-bit or fp32) -> fp32 NCHW, keeping channels [c_off, c_off+channels)."""
    _arg("nhwc_to_nchw", "src", src, _ACT, shape=(None,) * 4)
    B, H, W, Cs = src.shape
    Cc = Cs - c_off if channels is None else channels
    if c_off < 0 or Cc <= 0 or c_off + Cc > Cs:
        _bad("nhwc_to_nchw", "src", f"has {Cs} channels: the window [{c_off}, {c_off + Cc}) does not fit")
    _need_gpu(src)
    out = torch.empty((B, Cc, H, W), device=src.device, dtype=torch.float32)
    f32 = src.dtype == torch.float32
    L.check(L.load().rsvld_nhwc_to_nchw_f32(_ptr(src), _ptr(out), B, Cc, H, W, Cs, c_off, int(f32),
                                            0 if f32 else _dt(src), _stream()), "rsvld_nhwc_to_nchw_f32")
    return out


def axpby(a, b, sa=1.0, sb=1.0):
    _arg("axpby", "a", a, _ACT)
    _same("axpby", "b", b, a)
    _need_gpu(a, b)
    out = torch.empty_like(a)
    if a.dtype == torch.float32:
        L.check(L.load().rsvld_axpby_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), sa, sb, _stream()), "rsvld_axpby_f32")
        if a.dim() == 4:
            out._nhwc = True
        return out
    L.check(L.load().rsvld_axpby(_ptr(a), _ptr(b), _ptr(out), a.numel(), sa, sb, _dt(a), _stream()), "rsvld_axpby")
    return out


def geglu(x):
    # (16-bit only: the fp32 families fuse GEGLU into the projection's epilogue)
    _arg("geglu", "x", x, _HALF)
    if x.dim() < 1 or x.shape[-1] % 2:
        _bad("geglu", "x", f"must hold [value | gate] rows of an even width, got shape {tuple(x.shape)}")
    _need_gpu(x)
    Cc = x.shape[-1] // 2
    rows = x.numel() // x.shape[-1]
    out = torch.empty((*x.shape[:-1], Cc), device=x.device, dtype=x.dtype)
    L.check(L.load().rsvld_geglu(_ptr(x), _ptr(out), rows, Cc, _dt(x), _stream()), "rsvld_geglu")
    return out


def ddpm_step(x, eps_nhwc, noise, c_recip, c_recipm1, coef1, coef2, sigma, clip=True):
    """SR3 ancestral step on fp32 NCHW ``x`` with the UNet's fp32 NHWC eps (diffusion.py:142-175)."""
    _arg("ddpm_step", "x", x, torch.float32, shape=(None,) * 4)
    B, Cc, H, W = x.shape
    _arg("ddpm_step", "eps_nhwc", eps_nhwc, torch.float32, shape=(B, H, W, None))
    if eps_nhwc.shape[-1] < Cc:
        _bad("ddpm_step", "eps_nhwc", f"has {eps_nhwc.shape[-1]} channels, x {Cc}")
    _same("ddpm_step", "noise", noise, x, optional=True)
    _need_gpu(x, eps_nhwc, noise)
    out = torch.empty_like(x)
    L.check(L.load().rsvld_ddpm_step(_ptr(x), _ptr(eps_nhwc), _ptr(noise), _ptr(out), B, Cc, H, W,
                                     eps_nhwc.shape[-1], c_recip, c_recipm1, coef1, coef2, sigma, int(clip),
                                     _stream()), "rsvld_ddpm_step")
    return out


# ----------------------------------------------------------------------------- Stage-2 sampler / cache / VAE posterior
def denoiser_out(net_out_nhwc, inp, c_out, c_skip):
    """fp32 NHWC network output -> fp32 NCHW ``net*c_out + input*c_skip`` (denoiser.py:77-78)."""
    _arg("denoiser_out", "inp", inp, torch.float32, shape=(None,) * 4)
    B, Cc, H, W = inp.shape
    _arg("denoiser_out", "net_out_nhwc", net_out_nhwc, torch.float32, shape=(B, H, W, None))
    if net_out_nhwc.shape[-1] < Cc:
        _bad("denoiser_out", "net_out_nhwc", f"has {net_out_nhwc.shape[-1]} channels, the input {Cc}")
    _need_gpu(net_out_nhwc, inp)
    out = torch.empty_like(inp)
    L.check(L.load().rsvld_denoiser_out(_ptr(net_out_nhwc), _ptr(inp), _ptr(out), B, Cc, H, W, net_out_nhwc.shape[-1],
                                        c_out, c_skip, _stream()), "rsvld_denoiser_out")
    return out


def lerp_f32(a, b, w):
    _arg("lerp_f32", "a", a, torch.float32)
    _same("lerp_f32", "b", b, a)
    _need_gpu(a, b)
    out = torch.empty_like(a)
    L.check(L.load().rsvld_lerp_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), w, _stream()), "rsvld_lerp_f32")
    return out


def axpy_f32(x, y, s):
    """x + s*y on fp32 tensors; ``x=None`` gives s*y."""
    _arg("axpy_f32", "y", y, torch.float32)
    _same("axpy_f32", "x", x, y, optional=True)
    _need_gpu(x, y)
    out = torch.empty_like(y)
    L.check(L.load().rsvld_axpy_f32(_ptr(x), _ptr(y), _ptr(out), y.numel(), s, _stream()), "rsvld_axpy_f32")
    return out


def euler_step(x_hat, denoised, x_center, restore_w, sigma_hat, dt):
    _arg("euler_step", "x_hat", x_hat, torch.float32)
    _same("euler_step", "denoised", denoised, x_hat)
    _same("euler_step", "x_center", x_center, x_hat, optional=True)
    _need_gpu(x_hat, denoised, x_center)
    out = torch.empty_like(x_hat)
    L.check(L.load().rsvld_euler_step(_ptr(x_hat), _ptr(denoised), _ptr(x_center), _ptr(out), x_hat.numel(),
                                      restore_w, sigma_hat, dt, _stream()), "rsvld_euler_step")
    return out


def tile_blend_accumulate(acc, cnt, tile, weights, y0, x0):
    """In place: ``acc[:, :, y0:y0+th, x0:x0+tw] += tile * weights``, ``cnt[...] += weights`` (fp32 NCHW; sampling.py:733-734)."""
    fn = "tile_blend_accumulate"
    _arg(fn, "acc", acc, torch.float32, shape=(None,) * 4)
    B, Cc, H, W = acc.shape
    _same(fn, "cnt", cnt, acc)
    _arg(fn, "tile", tile, torch.float32, shape=(B, Cc, None, None))
    th, tw = tile.shape[-2:]
    _arg(fn, "weights", weights, torch.float32, shape=(th, tw))
    if not (0 <= int(y0) and int(y0) + th <= H and 0 <= int(x0) and int(x0) + tw <= W):
        _bad(fn, "tile", f"window [{y0}:{int(y0) + th}, {x0}:{int(x0) + tw}] lies outside the {H}x{W} latent")
    _need_gpu(acc, cnt, tile, weights)
    L.check(L.load().rsvld_tile_blend_accumulate(_ptr(acc), _ptr(cnt), _ptr(tile), _ptr(weights), B, Cc, H, W, int(y0), int(x0),
                                                 th, tw, _stream()), "rsvld_tile_blend_accumulate")


def tile_blend_finish(acc, cnt):
    """-> ``acc / cnt`` (sampling.py:735)."""
    _arg("tile_blend_finish", "acc", acc, torch.float32)
    _same("tile_blend_finish", "cnt", cnt, acc)
    _need_gpu(acc, cnt)
    out = torch.empty_like(acc)
    L.check(L.load().rsvld_tile_blend_finish(_ptr(acc), _ptr(cnt), _ptr(out), acc.numel(), _stream()), "rsvld_tile_blend_finish")
    return out


def absdiff_sums(a, b):
    """Per batch row: fp32 ``[rows, 2]`` = (sum|a-b|, sum|a|)  (DFBCache.py:98-112)."""
    _arg("absdiff_sums", "a", a, _ACT)
    if a.dim() < 1 or a.numel() == 0:
        _bad("absdiff_sums", "a", f"needs batch rows, got shape {tuple(a.shape)}")
    _same("absdiff_sums", "b", b, a)
    _need_gpu(a, b)
    rows = a.shape[0]
    n = a.numel() // rows
    lib = L.load()
    out = torch.empty((rows, 2), device=a.device, dtype=torch.float32)
    if a.dtype == torch.float32:
        L.check(lib.rsvld_absdiff_sums_f32(_ptr(a), _ptr(b), _ptr(out), rows, n, _stream()), "rsvld_absdiff_sums_f32")
        return out
    ws = torch.empty(lib.rsvld_absdiff_ws_bytes(rows, n), device=a.device, dtype=torch.uint8)
    L.check(lib.rsvld_absdiff_sums(_ptr(a), _ptr(b), _ptr(out), rows, n, _dt(a), _ptr(ws), _stream()),
            "rsvld_absdiff_sums")
    return out


def gaussian_sample(moments, channels, noise, scale):
    """NHWC moments (16-bit or fp32) -> fp32 NCHW z; ``noise=None`` gives mode()."""
    _arg("gaussian_sample", "moments", moments, _ACT, shape=(None,) * 4)
    B, H, W, mc = moments.shape
    if channels <= 0 or mc < 2 * channels:
        _bad("gaussian_sample", "moments", f"has {mc} channels, mean | logvar of {channels} need {2 * channels}")
    _arg("gaussian_sample", "noise", noise, torch.float32, shape=(B, channels, H, W), optional=True)
    _need_gpu(moments, noise)
    z = torch.empty((B, channels, H, W), device=moments.device, dtype=torch.float32)
    f32 = moments.dtype == torch.float32
    L.check(L.load().rsvld_gaussian_sample(_ptr(moments), _ptr(noise), _ptr(z), B, channels, H, W, mc, scale, int(f32),
                                           0 if f32 else _dt(moments), _stream()), "rsvld_gaussian_sample")
    return z


def wavelet_blur(img, radius, high_accum=None):
    """-> the dilated 3x3 blur of fp32 NCHW ``img``; ``high_accum`` (of ``img``'s shape) accumulates ``img - blur`` in place."""
    _arg("wavelet_blur", "img", img, torch.float32, shape=(None,) * 4)
    _same("wavelet_blur", "high_accum", high_accum, img, optional=True)
    _need_gpu(img, high_accum)
    B, Cc, H, W = img.shape
    low = torch.empty_like(img)
    L.check(L.load().rsvld_wavelet_blur(_ptr(img), _ptr(low), _ptr(high_accum), B * Cc, H, W, radius, _stream()),
            "rsvld_wavelet_blur")
    return low


def add_f32(a, b):
    _arg("add_f32", "a", a, torch.float32)
    _same("add_f32", "b", b, a)
    _need_gpu(a, b)
    out = torch.empty_like(a)
    L.check(L.load().rsvld_add_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), "rsvld_add_f32")
    return out


def adain(content, style):
    """Per (image, channel) plane: content normalised to the style's mean and (unbiased) standard deviation; fp32 NCHW of one shape."""
    _arg("adain", "content", content, torch.float32, shape=(None,) * 4)
    _same("adain", "style", style, content)
    _need_gpu(content, style)
    B, Cc, H, W = content.shape
    out = torch.empty_like(content)
    ws = torch.empty(4 * B * Cc, device=content.device, dtype=torch.float32)
    L.check(L.load().rsvld_adain(_ptr(content), _ptr(style), _ptr(out), _ptr(ws), B * Cc, H * W, _stream()),
            "rsvld_adain")
    return out


def concat_c(a, b):
    _arg("concat_c", "a", a, _ACT)
    if a.dim() < 1:
        _bad("concat_c", "a", "needs a channel dimension")
    _arg("concat_c", "b", b, a.dtype, shape=tuple(a.shape[:-1]) + (None,))
    _need_gpu(a, b)
    rows = a.numel() // a.shape[-1]
    out = torch.empty((*a.shape[:-1], a.shape[-1] + b.shape[-1]), device=a.device, dtype=a.dtype)
    if a.dtype == torch.float32:
        L.check(L.load().rsvld_concat_c_f32(_ptr(a), _ptr(b), _ptr(out), rows, a.shape[-1], b.shape[-1], _stream()), "rsvld_concat_c_f32")
        if a.dim() == 4:
            out._nhwc = True
        return out
    L.check(L.load().rsvld_concat_c(_ptr(a), _ptr(b), _ptr(out), rows, a.shape[-1], b.shape[-1], _dt(a), _stream()),
            "rsvld_concat_c")
    return out
