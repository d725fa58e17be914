"""Stage-1 (SR3) pixel-space UNet on the MI355X kernel library.

Drop-in for the reference ``models/sr3_model/sr3_modules/unet.py`` (UNet :162-261): same
constructor arguments, same parameter names (so ``I1000000_E800_gen.pth`` loads unchanged), same
``forward(x, time)`` contract.  What differs is everything underneath: activations are 16-bit
NHWC tensors that never leave HBM in NCHW form, and every layer is a kernel of librsvld_hip.so:

  Block            GN(32)+Swish (norm.hip) -> Conv3x3 implicit GEMM on MFMA (conv_igemm.hip)
  FeatureWiseAffine all 26 noise-level projections in ONE stacked launch (HipNet.emb_rows), consumed
                   as the per-image row vector of block1's conv epilogue
  ResnetBlock      residual / 1x1 res_conv add fused in block2's conv epilogue; the skip
                   concatenation (unet.py:257) is never materialised (two-source GN + conv)
  SelfAttention    fused qkv 1x1 GEMM -> flash attention, d = 512 (attention.hip) -> out 1x1 GEMM
                   with the residual in its epilogue; no [B,1,h,w,h,w] score tensor (:133-141)
  Upsample         nearest x2 folded into the conv's gather;  Downsample: stride-2 gather

The nn.Conv2d / nn.GroupNorm / nn.Linear children only HOLD parameters under the reference's
names; their ``forward`` is never called.  ``UNet`` is a ``hipnn.HipNet``: the precision record
(``compute_dtype``, ``pack_dtype``, ``split``, ``precision_key()``), the packed weights and their
life cycle (``pk``, ``packed``, ``pack_version``, ``invalidate_packed()``) are the base's, and each
layer fetches its weights where it uses them.  What is SR3's own is the parsing of the five
precision names and the two re-associated attention weights.
"""
import math

import torch
from torch import nn

from ... import ops
from ..._lib import RsvldError
from ...hipnn import HipNet


class PositionalEncoding(nn.Module):  # parameter-free; index 0 of noise_level_mlp (unet.py:19-32)
    def __init__(self, dim):
        super().__init__()
        self.dim = dim


class Swish(nn.Module):
    pass


class FeatureWiseAffine(nn.Module):
    """unet.py:35-51 — only the additive form is used by the shipped config."""

    def __init__(self, in_channels, out_channels, use_affine_level=False):
        super().__init__()
        if use_affine_level:
            raise NotImplementedError("use_affine_level=True is not used by configs/sr_sr3.json")
        self.use_affine_level = use_affine_level
        self.noise_func = nn.Sequential(nn.Linear(in_channels, out_channels))


class Upsample(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="nearest")
        self.conv = nn.Conv2d(dim, dim, 3, padding=1)


class Downsample(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv2d(dim, dim, 3, 2, 1)


class Block(nn.Module):
    def __init__(self, dim, dim_out, groups=32, dropout=0):
        super().__init__()
        self.block = nn.Sequential(
            nn.GroupNorm(groups, dim), Swish(),
            nn.Dropout(dropout) if dropout != 0 else nn.Identity(),
            nn.Conv2d(dim, dim_out, 3, padding=1))


class ResnetBlock(nn.Module):
    def __init__(self, dim, dim_out, noise_level_emb_dim=None, dropout=0, use_affine_level=False, norm_groups=32):
        super().__init__()
        self.noise_func = FeatureWiseAffine(noise_level_emb_dim, dim_out, use_affine_level)
        self.block1 = Block(dim, dim_out, groups=norm_groups)
        self.block2 = Block(dim_out, dim_out, groups=norm_groups, dropout=dropout)
        self.res_conv = nn.Conv2d(dim, dim_out, 1) if dim != dim_out else nn.Identity()

    @property
    def _emb_linear(self):  # picked up by HipNet.emb_rows
        return self.noise_func.noise_func[0]


class SelfAttention(nn.Module):
    def __init__(self, in_channel, n_head=1, norm_groups=32):
        super().__init__()
        self.n_head = n_head
        self.norm = nn.GroupNorm(norm_groups, in_channel)
        self.qkv = nn.Conv2d(in_channel, in_channel * 3, 1, bias=False)
        self.out = nn.Conv2d(in_channel, in_channel, 1)


class ResnetBlocWithAttn(nn.Module):
    def __init__(self, dim, dim_out, *, noise_level_emb_dim=None, norm_groups=32, dropout=0, with_attn=False):
        super().__init__()
        self.with_attn = with_attn
        self.res_block = ResnetBlock(dim, dim_out, noise_level_emb_dim, norm_groups=norm_groups, dropout=dropout)
        if with_attn:
            self.attn = SelfAttention(dim_out, norm_groups=norm_groups)


class UNet(HipNet):
    def __init__(self, in_channel=6, out_channel=3, inner_channel=32, norm_groups=32,
                 channel_mults=(1, 2, 4, 8, 8), attn_res=(8), res_blocks=3, dropout=0,
                 with_noise_level_emb=True, image_size=128):
        super().__init__()
        if not with_noise_level_emb:
            raise NotImplementedError("the SR3 sampler always conditions on the noise level")
        if isinstance(attn_res, int):
            attn_res = (attn_res,)
        self.in_channel, self.out_channel = in_channel, out_channel if out_channel is not None else in_channel
        emb = inner_channel
        self.noise_level_mlp = nn.Sequential(
            PositionalEncoding(inner_channel), nn.Linear(inner_channel, inner_channel * 4), Swish(),
            nn.Linear(inner_channel * 4, inner_channel))

        # encoder: attention sites depend on the CONSTRUCTION-time resolution only (unet.py:198,221)
        widths = [inner_channel * m for m in channel_mults]
        res, cur = image_size, inner_channel
        skips = [cur]
        downs = [nn.Conv2d(in_channel, inner_channel, kernel_size=3, padding=1)]
        for level, width in enumerate(widths):
            attn_here = res in attn_res
            for _ in range(res_blocks):
                downs.append(ResnetBlocWithAttn(cur, width, noise_level_emb_dim=emb, norm_groups=norm_groups,
                                                dropout=dropout, with_attn=attn_here))
                cur = width
                skips.append(cur)
            if level != len(widths) - 1:
                downs.append(Downsample(cur))
                skips.append(cur)
                res //= 2
        self.downs = nn.ModuleList(downs)
        self.mid = nn.ModuleList([
            ResnetBlocWithAttn(cur, cur, noise_level_emb_dim=emb, norm_groups=norm_groups, dropout=dropout, with_attn=True),
            ResnetBlocWithAttn(cur, cur, noise_level_emb_dim=emb, norm_groups=norm_groups, dropout=dropout, with_attn=False)])
        ups = []
        for level in reversed(range(len(widths))):
            width, attn_here = widths[level], res in attn_res
            for _ in range(res_blocks + 1):
                ups.append(ResnetBlocWithAttn(cur + skips.pop(), width, noise_level_emb_dim=emb, norm_groups=norm_groups,
                                              dropout=dropout, with_attn=attn_here))
                cur = width
            if level != 0:
                ups.append(Upsample(cur))
                res *= 2
        self.ups = nn.ModuleList(ups)
        self.final_conv = Block(cur, self.out_channel, groups=norm_groups)

    def set_compute_dtype(self, dt, policy=None):
        """fp16 (default) / bf16: 16-bit storage, fp32 accumulation; fp32: the fp32-operand kernel family (what the reference's
        own Stage 1 computes in: it runs without autocast); "split": fp32 tensors, matrix products on split operands (three 16-bit
        MFMAs per product) under ``policy`` (an ``ops.SplitPolicy``, default ``ops.UNET_POLICY``); "w2" (round 5): fp16 tensors like
        "fp16", but every weight as the fp16 PAIR [W_lo | W_hi] (dtype RSVLD_F16W2, two MFMAs per product) -- the rounding of the
        WEIGHTS is the whole distance of "fp16" from the reference's CPU path after T = 50 steps.
        Only parses: the rules (which packs are kept, what bumps ``pack_version``) are ``HipNet.set_precision``'s."""
        split = None
        if dt == "split":
            split = policy or ops.UNET_POLICY
            if not isinstance(split, ops.SplitPolicy):
                raise TypeError("set_compute_dtype: policy must be an rsvld_amd.ops.SplitPolicy")
        pack = torch.float32 if dt == "w2" else None
        dt = {"fp16": torch.float16, "w2": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32, "split": torch.float32}.get(dt, dt)
        if dt not in (torch.float16, torch.bfloat16, torch.float32):
            raise ValueError(f"compute_dtype {dt!r}: fp16, w2, bf16, fp32 or split")
        self.set_precision(dt, pack, split)

    # ------------------------------------------------------------------ re-associated attention weights
    # Single-head attention with keys and values taken from ONE tensor (csrc/attention.hip, "SH" note):
    #     softmax(q k^T / sqrt(C)) v,  q = n Wq^T, k = n Wk^T, v = n Wv^T   (unet.py:126-141, qkv without bias)
    #   = softmax((n Wq^T Wk) n^T / sqrt(C)) n  Wv^T
    # so the query projection becomes Wk^T Wq (one C x C conv instead of the 3C-wide qkv conv), the keys AND values are
    # the normalised input itself, and Wv moves into the output projection (W_out Wv).  Products in fp32 on the host.
    @staticmethod
    def _wq_wk_wv(at):
        if at.n_head != 1:
            raise NotImplementedError("SR3 SelfAttention is built with n_head=1 (unet.py:151)")
        if at.qkv.bias is not None:
            raise NotImplementedError("SR3 SelfAttention's qkv conv has no bias (unet.py:121)")
        w = at.qkv.weight.detach().to("cpu", torch.float32).flatten(1)          # [3C, C]
        C_ = w.shape[1]
        return w[:C_], w[C_:2 * C_], w[2 * C_:]

    def _pack_attn_q(self, at):
        wq, wk, _ = self._wq_wk_wv(at)
        return ops.pack_conv((wk.t() @ wq).contiguous(), None, self.pack_dtype, self._dev(at.qkv.weight))

    def _pack_attn_out(self, at):
        wv = self._wq_wk_wv(at)[2]
        wo = at.out.weight.detach().to("cpu", torch.float32).flatten(1)        # [C, C]
        return ops.pack_conv((wo @ wv).contiguous(), at.out.bias, self.pack_dtype, self._dev(at.out.weight))

    # ------------------------------------------------------------------ forward pieces
    def _block(self, blk, x, x2=None, **conv_kw):
        """GN(32)+Swish+Conv3x3 as ONE fused conv call: statistics pass + conv with the normalisation applied
        while the input patch is staged (ops.conv2d norm=...); the skip concat [x | x2] is never built."""
        gn = blk.block[0]
        return ops.conv2d(x, self.pk(blk.block[3]), x2=x2, norm=(gn.weight, gn.bias, gn.num_groups, gn.eps, True),
                          **conv_kw)

    def _resblock(self, layer, x, x2, rows):
        """``rows``: ``emb_rows`` of the noise-level embedding (every FeatureWiseAffine at once)."""
        rb = layer.res_block
        h = self._block(rb.block1, x, x2, rowvec=rows[id(rb)], stats=True)     # its output feeds block2's GroupNorm
        if isinstance(rb.res_conv, nn.Conv2d):
            split = None if x2 is None else (x.shape[-1], x2.shape[-1])     # decided at run time: skip concat or not
            res = ops.conv2d(x, self.pk(rb.res_conv, tag=split, cin_split=split), x2=x2, pad=0)
        else:
            res = x
        h = self._block(rb.block2, h, residual=res, stats=not layer.with_attn)   # ... and the next block's, unless attention follows
        if layer.with_attn:
            h = self._attention(layer.attn, h)
        return h

    def _attention(self, at, x):
        B, H, W, Cc = x.shape
        # (planes / out_planes: honoured in the split precision only -- n feeds the query conv and the attention, q the attention)
        n = ops.group_norm(x, at.norm.weight, at.norm.bias, at.norm.num_groups, at.norm.eps, planes=True)
        wq = self.packed(("attn_q", id(at)), self._pack_attn_q, at)
        q = ops.conv2d(n, wq, pad=0, out_planes=True).reshape(B, H * W, Cc)
        kv = n.reshape(B, H * W, Cc)              # keys and values are the normalised input itself (see _wq_wk_wv)
        o = ops.attention(q, kv, kv, heads=1, scale=1.0 / math.sqrt(Cc))  # scale uses the full channel count (unet.py:135)
        wo = self.packed(("attn_out", id(at)), self._pack_attn_out, at)
        return ops.conv2d(o.reshape(B, H, W, Cc), wo, pad=0, residual=x)

    def forward_nhwc(self, x, noise_level):
        """x: 16-bit NHWC ``[B,H,W,pad8(in_channel)]``; noise_level fp32 ``[B,1]`` -> fp32 NHWC eps
        ``[B,H,W,pad8(out_channel)]`` (channels beyond out_channel are zero)."""
        with self.precision():
            mlp = self.noise_level_mlp
            pe = ops.sinusoidal(noise_level, mlp[0].dim, 0)
            t = ops.linear_small(pe, mlp[1].weight, mlp[1].bias, 0, 1)   # Linear + Swish
            t = ops.linear_small(t, mlp[3].weight, mlp[3].bias)
            rows = self.emb_rows(t, act_in=0)

            feats = []
            for layer in self.downs:
                if isinstance(layer, ResnetBlocWithAttn):
                    x = self._resblock(layer, x, None, rows)
                elif isinstance(layer, Downsample):
                    x = ops.conv2d(x, self.pk(layer.conv), stride=2, pad=1)
                else:
                    x = ops.conv2d(x, self.pk(layer), pad=1)
                feats.append(x)
            for layer in self.mid:
                x = self._resblock(layer, x, None, rows)
            for layer in self.ups:
                if isinstance(layer, ResnetBlocWithAttn):
                    x = self._resblock(layer, x, feats.pop(), rows)
                else:
                    x = ops.conv2d(x, self.pk(layer.conv), pad=1, upsample=True, stats=True)
            return self._block(self.final_conv, x, out_f32=True)

    def forward(self, x, time):
        """Reference contract (unet.py:236-261): fp32 NCHW ``[B,in,H,W]``, ``time [B,1]`` -> fp32 NCHW."""
        if not x.is_cuda:
            raise RsvldError("SR3 UNet runs on the GPU only")
        xin = ops.nchw_to_nhwc(x, self.compute_dtype)
        eps = self.forward_nhwc(xin, time.float())
        return ops.nhwc_to_nchw(eps, channels=self.out_channel)
