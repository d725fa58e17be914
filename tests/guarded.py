"""Poisoned, guard-banded buffers for kernel tests (a helper module: nothing here is collected).

The kernels promise, in their comments, things about memory OUTSIDE their operands: a clamped lane "re-reads a valid address", a
row past the end is "never stored", a clamped key "carries P = 0".  Tensors from torch's caching allocator cannot show a broken
promise (the neighbour is slack or a dead tensor full of finite numbers).  Here every operand, output and workspace of a call
lives in a buffer of its own,

    [ front guard | payload | rear guard ]         every byte outside the payload = 0xFF

* 0xFF bytes are NaN as fp16, bf16, fp32, fp64 and e4m3 and -1 as an integer (``poison_is_nan``): one fill serves every operand type,
  and a stray read that reaches a result makes it non-finite (0 * NaN = NaN).
* the payload starts 256-byte aligned (the alignment of an allocator block, which vector loads may rely on) and ends FLUSH
  against the rear guard: the first byte past the last element is poison.  Aligned by over-allocating and offsetting, and
  asserted: torch's CPU allocator aligns to 64 bytes only, and the CPU tests of this module see the layout of the GPU runs.
* guard size = max(1 MiB, ``TILE_ROWS`` row pitches of the placed tensor), rounded up to 256 bytes.  A missing clamp lets a lane
  read or write up to one workgroup's rows past the end of an operand, so the poison must reach that far.  ``TILE_ROWS`` = 512:
  the tile edges of the kernels are 256 rows (gemm256, conv_igemm_256x32), 128 / 64 (the other implicit-GEMM tiles), 8 x 32 and
  16 x 32 pixels (conv_halo), 128 / 256 query rows and 64 keys (attn_d64b, the d = 512 kernels, split.hip), and -- the
  largest -- the 512 query rows one workgroup of attn_d64c walks (csrc/attention_d64c.inc, A6C_MIN_WG).

``Arena.place`` moves an operand in, ``torch_proxy`` makes ``rsvld_amd.ops`` allocate its outputs and workspaces in the arena
(ops.py allocates through the names ``torch.empty`` / ``empty_like`` / ``zeros`` only and hands ``data_ptr()`` to the C ABI), and
``Arena.verdict`` checks after the call, with integer compares on raw bytes (NaN != NaN):

  1. every guard of every buffer still holds 0xFF (first damaged byte: buffer, offset, distance from the payload);
  2. every operand payload -- the gaps of a strided view included -- is bit-identical to what was placed, except the elements a
     wrapper documents as updated in place (``inplace=`` mask of ``place``);
  3. every returned tensor is finite in every element: nothing left unwritten, no poison consumed;
  4. the returned tensors are bit-identical to those of the same call on ordinary tensors (``same_bits``).

``run_guarded`` then repeats the guarded run on a side stream behind a gate, with operands that arrive late (``run_streamed``): the
same four verdicts there show that every launch of the call went to the stream the wrapper handed to the library.

No kernel is ever made to misbehave for the sake of this module: tests/test_guarded_instrument.py shows on the CPU, with writes
through ``Region.raw``, that each verdict rejects what it is for."""
import contextlib
import math
import time
import types

import torch

POISON = 0xFF
ALIGN = 256
MIN_GUARD = 1 << 20
TILE_ROWS = 512
POISON_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn)


class GuardError(AssertionError):
    """A verdict failed; the message names the buffer and the byte."""


def poison_is_nan():
    """{dtype: True} if a run of 0xFF bytes reads as NaN in that type (torch's own casts, on the CPU); int32 must read -1."""
    raw = torch.full((16,), POISON, dtype=torch.uint8)
    res = {dt: bool(torch.isnan(raw.view(dt).float()).all()) for dt in POISON_DTYPES}
    res[torch.int32] = bool((raw.view(torch.int32) == -1).all())
    return res


def guard_bytes(pitch):
    """Guard size for a tensor whose rows are ``pitch`` bytes apart (module docstring)."""
    g = max(MIN_GUARD, TILE_ROWS * int(pitch))
    return (g + ALIGN - 1) // ALIGN * ALIGN


def _row_pitch(shape, strides, isz):
    if len(shape) < 2:
        return isz
    return max(int(strides[-2]), int(shape[-1])) * isz


def _byte_view(raw, shape, strides, off_bytes, isz):
    """The bytes of the elements of a strided view, as a uint8 view ``shape + (isz,)`` of the raw buffer."""
    return torch.as_strided(raw, tuple(shape) + (isz,), tuple(int(s) * isz for s in strides) + (1,), off_bytes)


class Region:
    """One buffer ``[guard | payload | guard]``.  ``raw``: the uint8 tensor; the payload is ``raw[start:end]``; ``view``: the tensor
    the kernels see.  ``kind``: "operand" (placed: verdict 2 applies) or "alloc" (an output or workspace of the proxy)."""

    def __init__(self, raw, start, end, guard, name, kind):
        self.raw, self.start, self.end, self.guard, self.name, self.kind = raw, start, end, guard, name, kind
        self.view = None
        self.placed = None        # operand: the payload bytes as placed
        self.may_change = None    # operand: uint8 mask over the payload, 1 = a byte the wrapper documents as updated in place
        self.is_data = None       # strided view: uint8 mask over the payload, 1 = a byte of an element (0: a gap)

    @property
    def payload(self):
        return self.raw[self.start:self.end]


class Arena:
    """``Arena()``: every buffer is filled and every operand copied on the current stream.  ``Arena(early, late)``: the arena of a
    streamed run (``run_streamed``).  The 0xFF fill of every buffer runs on ``early`` -- the stream that was current before the
    side stream ``late`` was entered, whose work is not held back by the gate -- and ``late`` waits for it; an operand placed
    before ``arrive()`` keeps a 0xFF payload until ``arrive()`` queues its copy on the current stream."""

    def __init__(self, early=None, late=None):
        assert (early is None) == (late is None)
        self.regions = []
        self.early, self.late = early, late
        self.pending = None if late is None else []     # operands whose payload has not been queued yet

    # ------------------------------------------------------------------ allocation
    def _region(self, nbytes, pitch, device, name, kind):
        guard = guard_bytes(pitch)
        if self.late is None:
            raw = torch.full((guard + ALIGN + nbytes + guard,), POISON, dtype=torch.uint8, device=device)
        else:      # poison at once, whatever the side stream is waiting for: a launch that strays from it finds 0xFF, not stale bytes
            with torch.cuda.stream(self.early):
                raw = torch.full((guard + ALIGN + nbytes + guard,), POISON, dtype=torch.uint8, device=device)
            self.late.wait_stream(self.early)
        start = guard + (-(raw.data_ptr() + guard)) % ALIGN
        r = Region(raw, start, start + nbytes, guard, name, kind)
        assert (raw.data_ptr() + start) % ALIGN == 0 and start >= guard and raw.numel() - r.end >= guard
        self.regions.append(r)
        return r

    def _typed(self, r, dtype, shape, strides=None, off=0):
        isz = dtype.itemsize
        if r.end == r.start:       # an empty payload (a zero-size workspace)
            flat = r.raw[r.start:r.start].view(dtype)
        else:
            assert r.start % isz == 0 and (r.end - r.start) % isz == 0
            flat = r.payload.view(dtype)
        if strides is None:
            return flat.view(tuple(shape))
        return torch.as_strided(flat, tuple(shape), tuple(strides), flat.storage_offset() + off)

    def empty(self, shape, dtype, device, name=None, zero=False):
        """A contiguous tensor of the arena (what the proxy's ``torch.empty`` returns): payload = poison, or zeros."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        strides = torch.empty(shape, dtype=dtype, device="meta").stride()
        r = self._region(n * dtype.itemsize, _row_pitch(shape, strides, dtype.itemsize), device,
                         name or f"alloc#{len(self.regions)}{list(shape)}", "alloc")
        if zero:
            r.payload.zero_()
        r.view = self._typed(r, dtype, shape)
        assert r.view.is_contiguous() and (r.view.numel() == 0 or r.view.data_ptr() % ALIGN == 0)
        return r.view

    def place(self, t, name, inplace=None, poison_gaps=False):
        """Copy ``t`` into the arena and return the equivalent view (same shape, strides and dtype).  A strided view comes with the
        whole span of storage it covers; ``poison_gaps`` fills the storage BETWEEN its elements with 0xFF instead (``place_view``).
        ``inplace``: None (a read-only operand), True (every element may change) or a bool tensor of ``t``'s shape (those may)."""
        isz = t.element_size()
        shape, strides = tuple(t.shape), tuple(t.stride())
        assert all(s >= 0 for s in strides)
        span = 0 if t.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        r = self._region(span * isz, _row_pitch(shape, strides, isz), t.device, name, "operand")
        dense = t.is_contiguous()
        r.placed = torch.full((span * isz,), POISON, dtype=torch.uint8, device=t.device)     # the payload as placed
        if span:
            if dense or poison_gaps:
                src = t.detach().contiguous().view(-1).view(torch.uint8).view(shape + (isz,))
                _byte_view(r.placed, shape, strides, 0, isz).copy_(src)
            else:
                src = torch.as_strided(t.detach(), (span,), (1,), t.storage_offset())
                r.placed.copy_(src.contiguous().view(torch.uint8))
        if self.pending is not None:
            self.pending.append(r)
        else:
            r.payload.copy_(r.placed)
        r.view = self._typed(r, t.dtype, shape, strides)
        assert r.view.shape == t.shape and r.view.stride() == t.stride() and r.view.dtype == t.dtype
        assert t.numel() == 0 or r.view.data_ptr() % ALIGN == 0
        if not dense:
            r.is_data = torch.zeros(span * isz, dtype=torch.uint8, device=t.device)
            _byte_view(r.is_data, shape, strides, 0, isz).fill_(1)
        if inplace is not None:
            r.may_change = torch.zeros(span * isz, dtype=torch.uint8, device=t.device)
            m = _byte_view(r.may_change, shape, strides, 0, isz)
            if inplace is True:
                m.fill_(1)
            else:
                m.copy_(inplace.to(device=t.device, dtype=torch.uint8).unsqueeze(-1).expand(m.shape))
        for attr in ("_nhwc",):
            if hasattr(t, attr):
                setattr(r.view, attr, getattr(t, attr))
        return r.view

    def arrive(self):
        """Streamed run: queue, on the current stream, the payload of every operand placed so far; later operands are copied at once."""
        for r in self.pending:
            r.payload.copy_(r.placed)
        self.pending = None

    def place_view(self, t, name, inplace=None):
        """``place`` for a view the wrappers accept (column slices of a fused tensor, a channel slice of a stacked one): the storage
        between its rows holds poison, not the neighbouring slices."""
        return self.place(t, name, inplace=inplace, poison_gaps=True)

    def owns(self, t):
        """Does ``t`` live in a payload of this arena?"""
        p = t.data_ptr()
        return any(r.raw.data_ptr() + r.start <= p <= r.raw.data_ptr() + r.end and r.raw.device == t.device for r in self.regions)

    # ------------------------------------------------------------------ verdicts
    def check_guards(self):
        """Verdict 1."""
        for r in self.regions:
            for side, lo, hi in (("front", 0, r.start), ("rear", r.end, r.raw.numel())):
                bad = r.raw[lo:hi] != POISON
                if bool(bad.any()):
                    i = lo + int(bad.nonzero()[0])
                    dist = r.start - i if side == "front" else i - r.end + 1
                    raise GuardError(f"guard damaged: buffer '{r.name}' ({r.kind}), raw byte {i} = {int(r.raw[i]):#04x} in the {side} guard, "
                                     f"{dist} byte(s) {'before' if side == 'front' else 'past'} the payload of {r.end - r.start} bytes")

    def check_operands(self):
        """Verdict 2."""
        for r in self.regions:
            if r.kind != "operand":
                continue
            bad = r.payload != r.placed
            if r.may_change is not None:
                bad &= r.may_change == 0
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                where = "a gap of the view" if r.is_data is not None and int(r.is_data[i]) == 0 else "an element"
                raise GuardError(f"operand modified: buffer '{r.name}', payload byte {i} ({where}) was {int(r.placed[i]):#04x}, "
                                 f"is {int(r.payload[i]):#04x}")

    def verdict(self, returned=None, plain=None, finite=None):
        """All four verdicts after ONE device synchronise.  ``returned`` / ``plain``: what the guarded and the plain call returned
        (tensors, Planes / Q8Rows, tuples; ``_gn_part`` riders are followed).  ``finite(name, tensor) -> bool tensor``: a case's own
        element test for a returned tensor whose bytes are not one float type (the e4m3 plane of Q8Rows)."""
        if any(r.raw.is_cuda for r in self.regions):
            torch.cuda.synchronize()
        self.check_guards()
        self.check_operands()
        if returned is not None:
            all_finite(returned, finite)
            if plain is not None:
                same_bits(returned, plain)


def tensors_of(obj, name="result"):
    """[(name, tensor)] of everything tensor-like inside a wrapper's return value, epilogue partials included."""
    out = []
    if obj is None:
        return out
    if isinstance(obj, torch.Tensor):
        out.append((name, obj))
        part = getattr(obj, "_gn_part", None)
        if part is not None:
            out.append((name + "._gn_part", part[0]))
        return out
    if hasattr(obj, "t") and isinstance(getattr(obj, "t"), torch.Tensor):     # ops.Planes / ops.Q8Rows
        return tensors_of(obj.t, name + ".t")
    if isinstance(obj, (tuple, list)):
        for i, o in enumerate(obj):
            out += tensors_of(o, f"{name}[{i}]")
        return out
    if isinstance(obj, dict):
        for k, o in obj.items():
            out += tensors_of(o, f"{name}[{k!r}]")
        return out
    raise TypeError(f"{name}: cannot look inside a {type(obj).__name__}")


def all_finite(returned, finite=None):
    """Verdict 3."""
    for name, t in tensors_of(returned):
        if t.numel() == 0:
            continue
        ok = finite(name, t) if finite is not None else None
        if ok is None:
            if not t.is_floating_point():
                raise TypeError(f"{name}: a returned {t.dtype} tensor needs the case's own element test")
            ok = torch.isfinite(t)
        if not bool(ok.all()):
            idx = tuple(int(v) for v in (~ok).nonzero()[0])
            raise GuardError(f"returned tensor '{name}' {tuple(t.shape)} {t.dtype}: element {idx} is not finite "
                             f"({int((~ok).sum())} such): left unwritten, or poison reached it")


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def same_bits(returned, plain):
    """Verdict 4."""
    a, b = tensors_of(returned), tensors_of(plain, "plain")
    if len(a) != len(b):
        raise GuardError(f"the guarded call returned {[n for n, _ in a]}, the plain call {[n for n, _ in b]}")
    for (name, x), (_, y) in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            raise GuardError(f"returned tensor '{name}': {tuple(x.shape)} {x.dtype} guarded, {tuple(y.shape)} {y.dtype} plain")
        d = _bits(x) != _bits(y)
        if bool(d.any()):
            i = int(d.nonzero()[0])
            raise GuardError(f"returned tensor '{name}' {tuple(x.shape)} {x.dtype} depends on what lies around its operands: byte {i} "
                             f"(element {i // x.element_size()}) is {int(_bits(x)[i]):#04x} guarded, {int(_bits(y)[i]):#04x} plain; "
                             f"{int(d.sum())} bytes differ")


# ---------------------------------------------------------------------- allocation proxy
class TorchProxy(types.ModuleType):
    """Stands in for the name ``torch`` inside a module: ``empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` return arena views,
    every other attribute is torch's own."""

    def __init__(self, arena):
        super().__init__("torch")
        self.__dict__["_arena"] = arena

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def _size(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(size[0])
        return tuple(size)

    def _new(self, size, dtype, device, zero, kw):
        if kw:
            raise TypeError(f"guarded torch proxy: unsupported allocation arguments {sorted(kw)}")
        return self._arena.empty(size, dtype or torch.get_default_dtype(), device, zero=zero)

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._new(self._size(size), dtype, device, False, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        return self._new(self._size(size), dtype, device, True, kw)

    def empty_like(self, t, dtype=None, device=None, **kw):
        return self._new(t.shape, dtype or t.dtype, device or t.device, False, kw)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        return self._new(t.shape, dtype or t.dtype, device or t.device, True, kw)


@contextlib.contextmanager
def torch_proxy(arena, modules=None):
    """Inside the block the name ``torch`` of ``rsvld_amd.ops`` (or of ``modules``) is a ``TorchProxy`` on ``arena``; restored on
    exit, an exception included."""
    if modules is None:
        from rsvld_amd import ops
        modules = (ops,)
    proxy = TorchProxy(arena)
    saved = [(m, m.torch) for m in modules]
    for m in modules:
        m.torch = proxy
    try:
        yield proxy
    finally:
        for m, t in saved:
            m.torch = t


# ---------------------------------------------------------------------- packed weights
PACKED_SLOTS = ("w", "bias", "w1", "w2", "w3", "wq8")


def relocate(pc, arena, name="pc"):
    """Move every tensor slot of a ``PackedConv`` that is not yet in the arena into it (in place on ``pc``).  The device-side packers
    (``ops._w2`` / ``_w3`` / ``_wq8``) run under the proxy BEFORE this, so their outputs already are guarded allocations."""
    for slot in PACKED_SLOTS:
        t = getattr(pc, slot)
        if t is not None and not arena.owns(t):
            setattr(pc, slot, arena.place(t, f"{name}.{slot}"))
    return pc


def copy_packed(pc):
    """A second ``PackedConv`` over the same master ``w`` / ``bias`` with no lazy form yet."""
    from rsvld_amd import ops
    return ops.PackedConv(pc.w, pc.bias, pc.cin, pc.cout, pc.cin_p, pc.cout_p, pc.kh, pc.kw, pc.geglu)


# ---------------------------------------------------------------------- launch recorder
class LaunchRecorder:
    """On the hook of ``ops.LaunchProfiler`` (``ops.tuning(profiler=...)``): the names ``_launch`` passes, no events."""

    def __init__(self):
        self.names = []

    def run(self, name, flops, nbytes, fn):
        self.names.append(name)
        return fn()

    def ran(self, prefix):
        """Was a kernel of exactly this name launched (the shape detail ``ops._detail`` may append does not count)?"""
        return any(n.split(" [")[0] == prefix for n in self.names)


# ---------------------------------------------------------------------- the runner
class Op:
    """One operand of a guarded case: ``value`` is a tensor, a Planes / Q8Rows, a PackedConv or a tuple of those (``norm=``).
    ``inplace``: see ``Arena.place``; ``view``: place with poisoned gaps; ``forms``: the lazy weight forms a PackedConv needs
    ("w1", "w2", "w3", "wq8"), packed under the proxy before the call."""

    def __init__(self, value, inplace=None, view=False, forms=()):
        self.value, self.inplace, self.view, self.forms = value, inplace, view, tuple(forms)


def _place_value(arena, v, name, op, later=None):
    """``later``: None, or the list of a streamed run: the lazy forms of a PackedConv are then packed by the thunk appended to it
    (behind the gate, from the late-arriving ``w`` of the arena) instead of at once."""
    from rsvld_amd import ops
    if v is None or isinstance(v, (int, float, bool, str)):
        return v
    if isinstance(v, torch.Tensor):
        if v.dim() == 0 and not v.is_floating_point() and not v.is_cuda:
            return v
        g = arena.place(v, name, inplace=op.inplace, poison_gaps=op.view)
        part = getattr(v, "_gn_part", None)
        if part is not None:
            g._gn_part = (arena.place(part[0], name + "._gn_part"), part[1])
        return g
    if isinstance(v, ops.Planes):
        return ops.Planes(_place_value(arena, v.t, name + ".t", op, later))
    if isinstance(v, ops.Q8Rows):
        return ops.Q8Rows(_place_value(arena, v.t, name + ".t", op, later))
    if isinstance(v, ops.PackedConv):
        g = copy_packed(v)
        packers = {"w1": ops._w1, "w2": ops._w2, "w3": ops._w3, "wq8": ops._wq8}

        def pack():
            with torch_proxy(arena):
                for f in op.forms:
                    packers[f](g)
            relocate(g, arena, name)
        if later is None:
            pack()
        else:
            relocate(g, arena, name)      # ``w`` / ``bias``: placed now, arriving late
            later.append(pack)
        return g
    if isinstance(v, (tuple, list)):
        return type(v)(_place_value(arena, e, f"{name}[{i}]", op, later) for i, e in enumerate(v))
    raise TypeError(f"operand '{name}': cannot place a {type(v).__name__}")


def _plain_value(v, op):
    """The operand of the plain call: the caller's own tensor; a private copy where the wrapper updates it in place."""
    if op.inplace is not None and isinstance(v, torch.Tensor):
        return v.clone()
    return v


def _place_all(arena, ops_, later=None):
    placed, seen = {}, {}
    for k, o in ops_.items():
        key = id(o.value)
        if key not in seen:
            seen[key] = _place_value(arena, o.value, k, o, later)
        placed[k] = seen[key]
    return placed


def _judge(arena, ops_, got, guarded_in, plain, plain_in, finite, compare_inplace):
    """The four verdicts of one guarded run against the plain run, the in-place operands and the packed forms included."""
    from rsvld_amd import ops
    for (name, t) in tensors_of(got):
        assert arena.owns(t) or t.numel() == 0, f"returned tensor '{name}' was not allocated through ops' torch.empty / zeros"
    arena.verdict(got, plain, finite)
    if compare_inplace:      # an operand updated in place ends as in the plain call, bit for bit
        for k, o in ops_.items():
            if o.inplace is not None and isinstance(o.value, torch.Tensor):
                same_bits({k: guarded_in[k]}, {k: plain_in[k]})
    for k, o in ops_.items():  # the device-side packers wrote every byte of the form they made, and the same bytes as outside the guard
        if isinstance(o.value, ops.PackedConv):
            for f in o.forms:
                a, b = getattr(guarded_in[k], f), getattr(plain_in[k], f)
                if b is not None:
                    same_bits({f"{k}.{f}": a}, {f"{k}.{f}": b})


def run_guarded(fn, operands, *, expect=None, finite=None, compare_inplace=True, streamed=None):
    """Place the operands, call ``fn(**operands)`` under the allocation proxy, call it on ordinary tensors, give the verdict; with
    device operands (or ``streamed=True``: a case that makes its device tensors itself) the same again on a gated side stream
    (``run_streamed``).  ``operands``: {name: tensor | Op | anything ``Op`` may hold}; identical objects (``k is v``) stay identical.
    ``expect``: name(s) of kernels that must have been launched (``LaunchRecorder``).  Returns (guarded result, recorder); the
    recorder carries the arena (``rec.arena``) and, after a streamed run, its record (``rec.streamed``)."""
    from rsvld_amd import ops
    ops_ = {k: (v if isinstance(v, Op) else Op(v)) for k, v in operands.items()}
    plain_in, seen = {}, {}
    for k, o in ops_.items():
        key = id(o.value)
        if key not in seen:
            seen[key] = _plain_value(o.value, o)
        plain_in[k] = seen[key]
    t0 = time.perf_counter()
    plain = fn(**plain_in)
    plain_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    arena = Arena()
    guarded_in = _place_all(arena, ops_)
    rec = LaunchRecorder()
    rec.arena = arena
    with torch_proxy(arena), ops.tuning(profiler=rec):
        got = fn(**guarded_in)
    host_ms = (time.perf_counter() - t0) * 1e3
    _judge(arena, ops_, got, guarded_in, plain, plain_in, finite, compare_inplace)
    if expect is not None:
        for e in ((expect,) if isinstance(expect, str) else expect):
            assert rec.ran(e), f"kernel '{e}' did not run; launched: {rec.names}"
    if streamed is None:
        streamed = any(_device_tensors(o.value) for o in ops_.values()) or any(t.is_cuda for _, t in tensors_of(got))
    if streamed:
        rec.streamed = run_streamed(fn, ops_, plain, plain_in, host_ms=host_ms, plain_ms=plain_ms, finite=finite,
                                    compare_inplace=compare_inplace, names=rec.names)
    return got, rec


# ---------------------------------------------------------------------- the streamed run
class Inconclusive(AssertionError):
    """The gate of a streamed run had finished before the host had queued the whole call: a launch on another stream would not have
    been told from one on the side stream, so the run proves nothing.  Never a pass, never a skip."""


GATE_N = 4096            # one link of the gate: an fp16 matrix product of this order (0.14 TFLOP)
GATE_MARGIN = 4.0        # gate = GATE_MARGIN x the host time of the case's guarded run + GATE_FLOOR_MS; then 4 x that, once
GATE_FLOOR_MS = 2.0
STREAM_LOG = []          # one record per streamed run of this process (the tests print them; a summary reads them)
_GATES, _SIDE = {}, {}


def side_stream(device):
    """THE side stream of this process on ``device``: one, so that no test run ever holds more than two streams."""
    key = torch.device(device).index or 0
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


class Gate:
    """A finite chain of fp16 matrix products on the current stream: plain torch work that ends by itself, whatever becomes of the
    test that queued it (no kernel here waits for a flag).  ``ms_per_link`` is measured once per process, with events."""

    def __init__(self, device):
        self.a = torch.full((GATE_N, GATE_N), 1.0 / GATE_N, dtype=torch.float16, device=device)
        self.b = torch.full((GATE_N, GATE_N), 1.0, dtype=torch.float16, device=device)
        self.c = torch.empty((GATE_N, GATE_N), dtype=torch.float16, device=device)
        self.queue(links=3)       # the library's own first-call work
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.queue(links=32)
        e1.record()
        e1.synchronize()
        self.ms_per_link = e0.elapsed_time(e1) / 32

    def queue(self, ms=None, links=None):
        links = max(1, math.ceil(ms / self.ms_per_link)) if links is None else links
        for _ in range(links):
            torch.mm(self.a, self.b, out=self.c)
        return links


def gate_for(device):
    key = torch.device(device).index or 0
    if key not in _GATES:
        _GATES[key] = Gate(device)
    return _GATES[key]


class StreamedRecorder(LaunchRecorder):
    """``LaunchRecorder`` that asks, after every launch is queued, whether the gate is still running."""

    def __init__(self, gate_done):
        super().__init__()
        self.gate_done, self.pending = gate_done, []

    def run(self, name, flops, nbytes, fn):
        self.names.append(name)
        out = fn()
        self.pending.append(not self.gate_done.query())
        return out


class GatedStream:
    """``with GatedStream(device, gate_ms) as g:`` -- inside the block THE side stream is current; it waits for the stream that was
    current before, then for a gate of about ``gate_ms`` (0: none).  ``g.pending()``: is the gate still running?"""

    def __init__(self, device, gate_ms):
        self.early, self.side, self.gate = torch.cuda.current_stream(device), side_stream(device), gate_for(device)
        assert self.side != self.early and self.side != torch.cuda.default_stream(device)
        self.want_ms, self.done, self.links = gate_ms, torch.cuda.Event(), 0

    def __enter__(self):
        self.side.wait_stream(self.early)
        self._ctx = torch.cuda.stream(self.side)
        self._ctx.__enter__()
        self.t0 = time.perf_counter()
        if self.want_ms > 0:
            self.links = self.gate.queue(ms=self.want_ms)
        self.done.record(self.side)
        return self

    @property
    def gate_ms(self):
        return self.links * self.gate.ms_per_link

    def pending(self):
        return not self.done.query()

    def __exit__(self, *exc):
        self.host_ms = (time.perf_counter() - self.t0) * 1e3
        return self._ctx.__exit__(*exc)


def _streamed_once(fn, ops_, gate_ms, device):
    """One streamed run -> (arena, operands as placed, result, recorder, was the gate pending throughout?, the GatedStream)."""
    from rsvld_amd import ops
    g = GatedStream(device, gate_ms)
    arena, later = Arena(g.early, g.side), []
    guarded_in = _place_all(arena, ops_, later)        # buffers poisoned, payloads staged: nothing has arrived
    with g:
        arena.arrive()                                  # the operands: behind the gate
        for pack in later:                              # the lazy weight forms: packed behind the gate, from what arrived
            pack()
        rec = StreamedRecorder(g.done)
        rec.arena = arena
        with torch_proxy(arena), ops.tuning(profiler=rec):
            got = fn(**guarded_in)
        pending = g.pending() and all(rec.pending)
    g.side.synchronize()
    return arena, guarded_in, got, rec, pending, g


def run_streamed(fn, ops_, plain, plain_in, *, host_ms, plain_ms=float("nan"), finite=None, compare_inplace=True, names=None,
                 gate_ms=None, device=None):
    """The guarded run again, on a side stream behind a gate.

    A second, non-blocking stream ``s`` waits for the current one; the first thing queued on it is the gate (``Gate``), sized from
    the host time of the case's own guarded run (``host_ms``: placement and call, the same host work as here; ``plain_ms``, the
    plain call's, is printed beside it -- it lacks the arena's allocations and, for the first call of a process, carries one-time
    costs).  Every buffer of a fresh arena is poisoned at once, but the operands' payloads are copied on ``s`` BEHIND the gate, the
    lazy PackedConv forms are packed there, and only then is ``fn`` called, inside ``torch.cuda.stream(s)``.  After
    ``s.synchronize()`` the four verdicts of ``run_guarded`` apply.

    What this catches: a launch that does not go to the stream ``ops._stream()`` hands to the library -- a dropped argument, a 0, the
    second launch of a multi-kernel op, a packer -- does not wait for the gate.  It reads operands that are still 0xFF, or a
    workspace its predecessor on ``s`` has not written, and a result is non-finite or differs from the plain run; if it only WRITES
    early, the late arrival or its successor on ``s`` overwrites it.  That needs no luck PROVIDED the gate is still running when
    the host has queued the whole call, which is checked: an event recorded behind the gate must be pending after every launch
    (``StreamedRecorder``) and after ``fn`` returns.  If it is not, the run is repeated ONCE with a gate four times as long; if
    it still is not, ``Inconclusive`` is raised -- a wrapper that synchronises the host inside the call always ends there."""
    if device is None:
        devs = [t.device for o in ops_.values() for _, t in _device_tensors(o.value)] + [t.device for _, t in tensors_of(plain) if t.is_cuda]
        device = devs[0] if devs else torch.device("cuda", torch.cuda.current_device())
    first = GATE_MARGIN * host_ms + GATE_FLOOR_MS if gate_ms is None else gate_ms
    tries = []
    for ms in (first, 4 * first):
        arena, guarded_in, got, rec, pending, g = _streamed_once(fn, ops_, ms, device)
        tries.append(dict(gate_ms=g.gate_ms, links=g.links, host_ms=g.host_ms, pending=pending))
        if pending:
            break
    log = dict(tries=tries, guarded_host_ms=host_ms, plain_ms=plain_ms, names=list(rec.names), conclusive=pending)
    STREAM_LOG.append(log)
    last = tries[-1]
    print(f"streamed: gate {last['gate_ms']:.2f} ms ({last['links']} links), host {last['host_ms']:.2f} ms (guarded run {host_ms:.2f} ms, "
          f"plain run {plain_ms:.2f} ms), {len(tries)} attempt(s), launched {rec.names}")
    if not pending:
        raise Inconclusive(f"the gate ({last['gate_ms']:.2f} ms, after {tries[0]['gate_ms']:.2f} ms) had finished before the call was queued "
                           f"(host {last['host_ms']:.2f} ms): the host waits for the stream inside the call?  launched {rec.names}, "
                           f"gate pending after each: {rec.pending}")
    if names is not None:
        assert rec.names == list(names), f"the streamed run launched {rec.names}, the guarded run {list(names)}"
    try:
        _judge(arena, ops_, got, guarded_in, plain, plain_in, finite, compare_inplace)
    except GuardError as e:
        raise GuardError(f"on a gated side stream (launched {rec.names}): {e}") from None
    return log


def _device_tensors(v):
    from rsvld_amd import ops
    if isinstance(v, torch.Tensor):
        return [("", v)] if v.is_cuda else []
    if isinstance(v, (ops.Planes, ops.Q8Rows)):
        return _device_tensors(v.t)
    if isinstance(v, ops.PackedConv):
        return _device_tensors(v.w)
    if isinstance(v, (tuple, list)):
        return [p for e in v for p in _device_tensors(e)]
    return []
