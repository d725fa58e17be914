"""Runtime shared by every network of the package (Stage 1: the SR3 UNet; Stage 2: UNet, ControlNet, VAE halves): the precision
record, the lazily packed kernel operands with their life cycle, and the stacked embedding projection.

A ``HipNet`` is the root nn.Module of one network.  Its layers are plain parameter containers
named like the reference's (so reference checkpoints load unchanged); the code that runs them
(Stage 2: their ``run(rt, ...)`` methods, which take the root as ``rt``; Stage 1: the root's own
methods) fetches each operand from the root where it uses it -- ``pk`` / ``pk_cat`` / ``packed`` --
and issues kernels of librsvld_hip.so through ``rsvld_amd.ops``.  Nothing is packed ahead of time:
the first (eager) forward packs, and whoever captures a forward into a hipGraph runs one first.
"""
import torch
from torch import nn

from . import ops
from ._lib import RsvldError


def precision(compute_dtype, split):
    """The launch context of a network whose operand type is ``compute_dtype``: the split precision under the policy ``split``
    when the tensors are fp32, else nothing.  (A function, because ``ControlWrapper`` holds a dtype and a policy without being a
    network root; every root enters it as ``self.precision()``.)"""
    return ops.f32_split(split if compute_dtype == torch.float32 else None)


class HipNet(nn.Module):
    # ---- the precision record.  ``compute_dtype`` may also be assigned directly (a class default, a test): ``pack_dtype`` follows it.
    compute_dtype = torch.float16   # storage / MFMA operand type of the activations
    _pack_dtype = None              # set only where the weights are packed in another type than ``compute_dtype``
    split = None                    # with compute_dtype fp32: the ops.SplitPolicy of the split precision, else None
    cache_context_kv = True   # reuse cross-attention K/V while the SAME context tensor object is passed

    def __init__(self):
        super().__init__()
        self._pk = {}
        self._pk_other = {}      # packed weights of the (compute_dtype, pack_dtype) pairs this network was switched away from

    @property
    def pack_dtype(self):
        """Type the weights are packed in: ``compute_dtype``, or fp32 masters under fp16 activations (SR3's "w2")."""
        return self._pack_dtype or self.compute_dtype

    def precision_key(self):
        return (str(self.compute_dtype), str(self.pack_dtype), None if self.split is None else self.split.key())

    def precision(self):
        return precision(self.compute_dtype, self.split)

    def set_precision(self, compute_dtype, pack_dtype=None, split=None):
        """Switch the whole record.  The packs of the (compute, pack) dtype pair switched away from are kept, so switching back and
        forth (precision A/B runs, tests) packs each once; "fp16" and "w2" share a compute dtype and never share packs.  ``split``
        chooses kernels, not packs (the masters are fp32 either way): a change of it alone drops nothing.  Every change bumps
        ``pack_version`` -- captured hipGraphs bake the mode in -- and a call that changes nothing bumps nothing."""
        old, new = (self.compute_dtype, self.pack_dtype), (compute_dtype, pack_dtype or compute_dtype)
        if new == old and split == self.split:
            return
        if new != old:
            self._pk_other[old] = self._pk
            self._pk = self._pk_other.pop(new, {})
            self.compute_dtype, self._pack_dtype = compute_dtype, (new[1] if new[1] != compute_dtype else None)
        self.split = split
        self.pack_version += 1

    def set_compute_dtype(self, dt):
        """Switch the operand type (fp16 / bf16: 16-bit kernels, fp32: the fp32-operand family); ``split`` stays as assigned."""
        self.set_precision(dt, None, self.split)

    # ---- cache invalidation whenever the fp32 master parameters move or change.  ``pack_version`` counts them: captured
    # hipGraphs hold raw pointers into the packed tensors and key themselves on it.
    pack_version = 0

    def invalidate_packed(self):
        self._pk = {}
        self._pk_other = {}
        self.pack_version += 1

    def load_state_dict(self, *a, **k):
        self.invalidate_packed()
        return super().load_state_dict(*a, **k)

    def _load_from_state_dict(self, *a, **k):   # reached when a PARENT module's load_state_dict recurses into this one
        self.invalidate_packed()
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):  # .to(device) / .half() etc. move the fp32 masters
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    # ---- packing
    def _dev(self, t):
        if t.device.type != "cuda":
            raise RsvldError(f"{type(self).__name__}: parameters must be on the GPU (there is no CPU execution path)")
        return t.device

    def packed(self, key, build, *args):
        """The one get-or-build of the cache: ``build(*args)`` runs on first use under the current precision."""
        p = self._pk.get(key)
        if p is None:
            p = self._pk[key] = build(*args)
        return p

    # (``pk`` / ``pk_cat`` look the key up themselves before they go through ``packed``, and hold no closure: a hit costs one dict
    #  lookup.  Measured: the tiled VAE is bound by the host, ~25 000 lookups per 4096^2 image; 260 ns more per hit were 6 ms.)
    def pk(self, m, tag="", **kw):
        """PackedConv of a Conv2d / Linear ``m`` (packed on first use)."""
        key = (id(m), tag)
        p = self._pk.get(key)
        if p is None:
            p = self.packed(key, self._pack_one, m, kw)
        return p

    def _pack_one(self, m, kw):
        return ops.pack_conv(m.weight, m.bias, self.pack_dtype, self._dev(m.weight), **kw)

    def pk_cat(self, mods, tag, **kw):
        """One PackedConv for several Linear/Conv layers that share their input (rows concatenated):
        q|k|v of a self-attention, k|v of a cross-attention, gamma|beta of ZeroSFT."""
        key = (tuple(id(m) for m in mods), tag)
        p = self._pk.get(key)
        if p is None:
            p = self.packed(key, self._pack_cat, mods, kw)
        return p

    def _pack_cat(self, mods, kw):
        w = torch.cat([m.weight.detach().float() for m in mods], 0)      # (stays on the masters' device: pack_conv re-lays it there)
        if all(m.bias is None for m in mods):
            b = None
        else:
            b = torch.cat([torch.zeros(m.weight.shape[0], device=w.device) if m.bias is None else m.bias.detach().float()
                           for m in mods], 0)
        return ops.pack_conv(w, b, self.pack_dtype, self._dev(mods[0].weight), **kw)

    # ---- stacked emb projections: the embedding Linear of every block that names one (``_emb_linear``) in ONE launch
    def emb_rows(self, emb, act_in=1):
        """emb fp32 [B, E] -> {id(block): fp32 view [B, Cout]} = Linear(act(emb)) for all blocks, stacked in module registration
        order.  ``act_in``: 1 = SiLU (Stage 2's ``emb_layers``), 0 = none (SR3's FeatureWiseAffine)."""
        def build():
            offs, ws, bs, off = {}, [], [], 0
            for m in self.modules():
                lin = getattr(m, "_emb_linear", None)
                if lin is not None:
                    offs[id(m)] = (off, lin.out_features)
                    ws.append(lin.weight.detach().float())
                    bs.append(lin.bias.detach().float())
                    off += lin.out_features
            dev = self._dev(ws[0])
            return torch.cat(ws, 0).contiguous().to(dev), torch.cat(bs, 0).contiguous().to(dev), offs
        w, b, offs = self.packed("emb_stack", build)
        table = ops.linear_small(emb, w, b, act_in=act_in)
        return {k: table[:, o:o + n] for k, (o, n) in offs.items()}
