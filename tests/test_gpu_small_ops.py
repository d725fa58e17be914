"""Parity of the small kernels around the big ones against a float64 torch reference of the same operation on the same rounded inputs,
at the shapes where they go wrong: every LayerNorm instantiation past its grid cap (the grid-stride row loop), the cache decision's
absdiff past its 256-chunk cap, the posterior's 16-bit moments and clamp edges, the sampler's element-wise updates past the 4096-block
grid, the wavelet blur's clamped dilations, AdaIN's ragged planes, the tile blend's overlapping windows, the bf16 and grid-stride forms
of the layout kernels and the ragged tiny linear layers.

Bounds (the measured figure is printed next to each):
  16-bit outputs       one output ulp of the fp64 value, plus the fp32 arithmetic before the rounding
  fp32 element-wise    a few fp32 ulps of the magnitude of the terms
  fp64-merged sums     1e-6 relative (absdiff, AdaIN)
Every bound is also shown to reject a host-side perturbation of the reference (the kind of bug it is there to catch)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def _ulp(ref, dtype):
    """Spacing of ``dtype`` at |ref| (fp64 tensor): 2^(exponent - mantissa bits), subnormals included."""
    fi = torch.finfo(dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(fi.tiny)))
    return torch.exp2(e - mant)


def _check(what, got, ref, bound):
    """max |got - ref| / bound <= 1 (all fp64 on the device); prints the measured figure."""
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"{what}: max|d| = {float(err.max()):.3e}, max|d|/bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max|d|/bound = {ratio:.3f}"
    return ratio


def _rejects(got, ref, bound):
    return bool(((got.double() - ref).abs() > bound).any())


def _rt(x, dtype):
    return x.to(dtype)


# ----------------------------------------------------------------------------- LayerNorm (16-bit), every instantiation past its grid cap
# launch_layernorm: <2,4> C <= 1024 (cap 65 536 rows), <3,3> C <= 1536 (49 152), <4,2> C <= 2048 (32 768), <8,1> C <= 4096 (16 384)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Cc,rows", [(1024, 65536 + 777), (1288, 49152 + 555), (2048, 32768 + 333), (4096, 16384 + 111)])
def test_layer_norm_bands_past_grid_cap(cuda, dtype, Cc, rows):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(Cc)
    x = _rt(torch.randn(rows, Cc, generator=g, device=cuda) * 1.5 + 0.3, dtype)
    gamma = 1 + 0.1 * torch.randn(Cc, generator=g, device=cuda)
    beta = 0.1 * torch.randn(Cc, generator=g, device=cuda)
    got = ops.layer_norm(x, gamma, beta, 1e-5)
    ref = F.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
    bound = _ulp(ref, dtype) + 64 * EPS32 * (ref.abs() + 1)
    _check(f"layer_norm {dtype} {rows}x{Cc}", got, ref, bound)
    # a kernel that stopped after its first grid pass leaves the tail rows unwritten: rejected
    bad = got.clone()
    bad[rows - 1] = 0
    assert _rejects(bad, ref, bound)


# ----------------------------------------------------------------------------- LayerNorm (split precision), past the 768-block cap
@pytest.mark.parametrize("Cc", [1024, 1288, 2048, 4096])
@pytest.mark.parametrize("form", ["f32", "planes", "f16"])
def test_layer_norm_split_bands_past_grid_cap(cuda, Cc, form):
    from rsvld_amd import ops
    rows = 6144 + 357        # the row loop starts at 6 144 (C <= 1 536) / 3 072 rows
    g = torch.Generator(device=cuda).manual_seed(Cc + 1)
    x = torch.randn(rows, Cc, generator=g, device=cuda) * 2 + 0.5
    gamma, beta = torch.randn(Cc, generator=g, device=cuda), torch.randn(Cc, generator=g, device=cuda)
    ref = F.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
    mag = ((x.double() - x.double().mean(-1, keepdim=True)) / x.double().std(-1, keepdim=True) * gamma.double()).abs() + beta.double().abs()
    fp32 = 64 * EPS32 * (mag + 1)
    if form == "f32":
        with ops.f32_split(ops.ALL_SPLIT):
            got = ops.layer_norm(x, gamma, beta, 1e-5)
        bound = fp32
    elif form == "planes":
        with ops.f32_split(ops.ALL_SPLIT):
            got = ops.layer_norm(x, gamma, beta, 1e-5, planes=True).f32()
        bound = 2.0 ** -16 * ref.abs() + fp32      # hi + lo: 16 significant bits
    else:
        with ops.f32_split(ops.UNET_POLICY):
            got = ops.layer_norm(x, gamma, beta, 1e-5, planes=True, group="qkv")
        assert got.dtype == torch.float16
        bound = _ulp(ref, torch.float16) + fp32
    _check(f"layer_norm_split {form} {rows}x{Cc}", got, ref, bound)
    bad = got.double().clone()
    bad[rows - 1] = 0
    assert _rejects(bad, ref, bound)


# ----------------------------------------------------------------------------- absdiff_sums (16-bit): the feature cache's decision
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,n", [(2, 320 * 128 * 128), (2, 4194304 + 8 * 2049 * 13), (3, 24)])
def test_absdiff_sums_16bit(cuda, dtype, rows, n):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(n)
    a = _rt(torch.randn(rows, n, generator=g, device=cuda), dtype)
    b = _rt(a.float() + 0.05 * torch.randn(rows, n, generator=g, device=cuda), dtype)
    got = ops.absdiff_sums(a, b)
    ad, bd = a.double(), b.double()
    ref = torch.stack([(ad - bd).abs().sum(1), ad.abs().sum(1)], 1)
    bound = 1e-6 * ref.abs()
    _check(f"absdiff_sums {dtype} {rows}x{n}", got, ref, bound)
    # a row whose last chunk is dropped (n8 / 256 vectors of 8 past the cap, or the last vector of a small row): rejected
    n8 = n // 8
    chunk8 = -(-n8 // min(256, -(-n8 // 2048)))
    nchunks = -(-n8 // chunk8)
    last = 8 * (n8 - (nchunks - 1) * chunk8 if nchunks > 1 else 1)
    short = torch.stack([(ad[:, :n - last] - bd[:, :n - last]).abs().sum(1), ad[:, :n - last].abs().sum(1)], 1)
    assert _rejects(short, ref, bound)


# ----------------------------------------------------------------------------- gaussian_sample: moments of every type, clamp edges
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("with_noise", [True, False])
def test_gaussian_sample(cuda, dtype, with_noise):
    from rsvld_amd import ops
    B, H, W, Cc, mc = 2, 5, 37, 4, 12     # m_c > 2 C: trailing channels the kernel must skip
    g = torch.Generator(device=cuda).manual_seed(3)
    mom = torch.randn(B, H, W, mc, generator=g, device=cuda)
    mom[..., Cc:2 * Cc] = mom[..., Cc:2 * Cc] * 4
    mom[0, 0, :5, Cc] = -40.0              # below the -30 clamp
    mom[0, 1, :5, Cc + 1] = 30.0           # above the +20 clamp
    mom[1, 2, :5, Cc + 2] = -30.0          # on the edges
    mom[1, 3, :5, Cc + 3] = 20.0
    mom = _rt(mom, dtype)
    noise = torch.randn(B, Cc, H, W, generator=g, device=cuda) if with_noise else None
    got = ops.gaussian_sample(mom, Cc, noise, 0.18215)
    md = mom.double().permute(0, 3, 1, 2)
    mean, lv = md[:, :Cc], md[:, Cc:2 * Cc]
    if with_noise:
        std = torch.exp(0.5 * lv.clamp(-30.0, 20.0))
        ref = (mean + std * noise.double()) * 0.18215
        mag = (mean.abs() + std * noise.double().abs()) * 0.18215
    else:
        ref, mag = mean * 0.18215, mean.abs() * 0.18215
    bound = 8 * EPS32 * mag + 1e-30
    _check(f"gaussian_sample {dtype} noise={with_noise}", got, ref, bound)
    if with_noise:   # the un-clamped logvar: rejected
        assert _rejects((mean + torch.exp(0.5 * lv) * noise.double()) * 0.18215, ref, bound)


# ----------------------------------------------------------------------------- Stage-2 sampler element-wise ops (fp32)
SHAPE = (2, 4, 400, 333)     # 1 065 600 elements: past the 4096 x 256 grid


def _rand(g, cuda, shape=SHAPE, s=1.0):
    return torch.randn(shape, generator=g, device=cuda) * s


def test_sampler_elementwise(cuda):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(11)
    a, b, c = _rand(g, cuda), _rand(g, cuda, s=3.0), _rand(g, cuda, s=0.5)
    ad, bd, cd = a.double(), b.double(), c.double()
    k = 4 * EPS32

    ref = ad + 7.5 * (bd - ad)
    _check("lerp_f32", ops.lerp_f32(a, b, 7.5), ref, k * (ad.abs() + 7.5 * (ad.abs() + bd.abs())))
    _check("axpy_f32", ops.axpy_f32(a, b, -0.3), ad - 0.3 * bd, k * (ad.abs() + 0.3 * bd.abs()))
    _check("axpy_f32 x=None", ops.axpy_f32(None, b, 1.7), 1.7 * bd, k * 1.7 * bd.abs() + 1e-30)
    _check("add_f32", ops.add_f32(a, b), ad + bd, k * (ad.abs() + bd.abs()) + 1e-30)
    sig, dt, w = 2.5, -0.4, 0.3
    for center in (None, c):
        if center is None:
            dn, dmag = bd, bd.abs()
        else:
            dn, dmag = bd - (bd - cd) * w, bd.abs() + (bd.abs() + cd.abs()) * w
        ref = ad + (ad - dn) / sig * dt
        mag = ad.abs() + (ad.abs() + dmag) / sig * abs(dt)
        got = ops.euler_step(a, b, center, w, sig, dt)
        _check(f"euler_step center={center is not None}", got, ref, 2 * k * mag)
        if center is not None:   # the restore pull dropped: rejected
            assert _rejects(ops.euler_step(a, b, None, w, sig, dt), ref, 2 * k * mag)
    # denoiser_out: NHWC network output with padded channels (c_pad = 8 > C = 4) -> NCHW
    net = torch.randn(2, 400, 333, 8, generator=g, device=cuda)
    ref = net.double()[..., :4].permute(0, 3, 1, 2) * 0.7 + ad * 0.2
    got = ops.denoiser_out(net, a, 0.7, 0.2)
    _check("denoiser_out c_pad 8 > C 4", got, ref, k * (net.double()[..., :4].permute(0, 3, 1, 2).abs() * 0.7 + ad.abs() * 0.2) + 1e-30)
    assert _rejects(net.double()[..., 4:].permute(0, 3, 1, 2) * 0.7 + ad * 0.2, ref, k * (ad.abs() + 1))


def test_tile_blend(cuda):
    """Two overlapping windows accumulated in turn, the second flush with the bottom-right corner; then acc / cnt."""
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(5)
    B, Cc, H, W, th, tw = 2, 4, 40, 56, 24, 32
    acc = torch.zeros(B, Cc, H, W, device=cuda)
    cnt = torch.zeros(B, Cc, H, W, device=cuda)
    ref_acc = acc.double().clone()
    ref_cnt = cnt.double().clone()
    for y0, x0 in ((3, 5), (H - th, W - tw)):
        tile = torch.randn(B, Cc, th, tw, generator=g, device=cuda)
        wts = torch.rand(th, tw, generator=g, device=cuda) + 0.1
        ops.tile_blend_accumulate(acc, cnt, tile, wts, y0, x0)
        ref_acc[:, :, y0:y0 + th, x0:x0 + tw] += tile.double() * wts.double()
        ref_cnt[:, :, y0:y0 + th, x0:x0 + tw] += wts.double()
    covered = ref_cnt > 0
    _check("tile_blend_accumulate acc", acc, ref_acc, 4 * EPS32 * (ref_acc.abs() + 2 * 4.0 * ref_cnt) + 1e-30)
    _check("tile_blend_accumulate cnt", cnt, ref_cnt, 4 * EPS32 * ref_cnt + 1e-30)
    cnt_safe = torch.where(covered, cnt, torch.ones_like(cnt))
    out = ops.tile_blend_finish(acc, cnt_safe)
    ref = acc.double() / cnt_safe.double()
    _check("tile_blend_finish", out, ref, 2 * EPS32 * ref.abs() + 1e-30)
    # the second window accumulated one row too high (not flush with the corner): rejected
    shifted = ref_acc.clone()
    shifted[:, :, H - 1] = 0
    assert _rejects(shifted, ref_acc, 4 * EPS32 * (ref_acc.abs() + 2 * 4.0 * ref_cnt) + 1e-30)


# ----------------------------------------------------------------------------- wavelet blur, AdaIN (utils/colorfix.py)
def _blur_ref(img, r):
    H, W = img.shape[-2:]
    ys, xs = torch.arange(H, device=img.device), torch.arange(W, device=img.device)
    out = torch.zeros_like(img)
    for dy, wy in ((-r, 1), (0, 2), (r, 1)):
        for dx, wx in ((-r, 1), (0, 2), (r, 1)):
            yi, xi = (ys + dy).clamp(0, H - 1), (xs + dx).clamp(0, W - 1)
            out += wy * wx / 16.0 * img[..., yi, :][..., xi]
    return out


@pytest.mark.parametrize("shape", [(1, 3, 9, 300), (2, 2, 33, 17), (1, 1, 1, 513)])   # W > 256; radius 16 >= H or W
def test_wavelet_blur_levels(cuda, shape):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(shape[-1])
    img = torch.rand(shape, generator=g, device=cuda) * 2 - 0.5
    high = torch.zeros_like(img)
    cur, ref_cur, ref_high, mag = img, img.double(), torch.zeros_like(img, dtype=torch.float64), img.double().abs()
    for i in range(5):                                        # wavelet_decomposition: radii 1, 2, 4, 8, 16
        low = ops.wavelet_blur(cur, 2 ** i, high_accum=high)
        ref_low = _blur_ref(ref_cur, 2 ** i)
        _check(f"wavelet_blur {shape} r={2 ** i} low", low, ref_low, 8 * EPS32 * _blur_ref(mag, 2 ** i) + 1e-30)
        ref_high += ref_cur - ref_low
        mag = _blur_ref(mag, 2 ** i) + 1e-30
        cur, ref_cur = low, low.double()                      # the next level blurs the kernel's own low pass
    _check(f"wavelet_blur {shape} high_accum", high, ref_high, 64 * EPS32 * img.double().abs().max())
    # un-clamped (zero) padding at the borders: rejected
    zp = F.conv2d(F.pad(img.double().reshape(-1, 1, *shape[-2:]), (1, 1, 1, 1)),
                  torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]], dtype=torch.float64, device=cuda)[None, None] / 16).reshape(shape)
    assert _rejects(zp, _blur_ref(img.double(), 1), 8 * EPS32 * _blur_ref(img.double().abs(), 1) + 1e-30)


@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (1, 4, 1, 2), (1, 2, 64, 64)])    # HW = 323 (not a multiple of 256), HW = 2
def test_adain(cuda, shape):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(shape[2])
    c = torch.randn(shape, generator=g, device=cuda) * 2 + 1
    s = torch.randn(shape, generator=g, device=cuda) * 0.5 - 3
    got = ops.adain(c, s)
    cd, sd = c.double().flatten(2), s.double().flatten(2)
    cm, sm = cd.mean(-1, keepdim=True), sd.mean(-1, keepdim=True)
    cs, ss = (cd.var(-1, keepdim=True) + 1e-5).sqrt(), (sd.var(-1, keepdim=True) + 1e-5).sqrt()
    ref = ((cd - cm) / cs * ss + sm).reshape(shape)
    bound = 1e-6 * (((cd - cm) / cs * ss).abs() + sm.abs()).reshape(shape)
    _check(f"adain {shape}", got, ref, bound)
    biased = ((cd - cm) / (cd.var(-1, keepdim=True, unbiased=False) + 1e-5).sqrt() * ss + sm).reshape(shape)   # biased variance: rejected
    assert _rejects(biased, ref, bound)


# ----------------------------------------------------------------------------- 16-bit layout / element-wise kernels: bf16, grid-stride
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_geglu_axpby_concat_grid_stride(cuda, dtype):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(7)
    # geglu: 6 600 x 1 280 outputs = 1 056 000 vectors of 8 (> 4096 x 256)
    x = _rt(torch.randn(6600, 2 * 1280, generator=g, device=cuda), dtype)
    got = ops.geglu(x)
    v, gt = x.double()[:, :1280], x.double()[:, 1280:]
    ref = v * 0.5 * gt * (1 + torch.erf(gt / math.sqrt(2)))
    bound = _ulp(ref, dtype) + 16 * EPS32 * v.abs() * gt.abs()
    _check(f"geglu {dtype} 6600x1280", got, ref, bound)
    tail = got.clone()
    tail[-1] = 0                 # the grid-stride loop's last pass missing: rejected
    assert _rejects(tail, ref, bound)
    # axpby: 9 000 000 elements
    a = _rt(torch.randn(2, 4500, 1000, generator=g, device=cuda), dtype)
    b = _rt(torch.randn(2, 4500, 1000, generator=g, device=cuda), dtype)
    got = ops.axpby(a, b, 0.7, 0.3)
    ref = 0.7 * a.double() + 0.3 * b.double()
    bound = _ulp(ref, dtype) + 4 * EPS32 * (0.7 * a.double().abs() + 0.3 * b.double().abs())
    _check(f"axpby {dtype} 9e6", got, ref, bound)
    last = got.clone().reshape(-1)
    last[-1] = -last[-1] if last[-1] != 0 else 1
    assert _rejects(last.reshape(got.shape), ref, bound)
    # concat_c: 9 000 rows x (640 + 384) channels = 1 152 000 vectors of 8: exact
    p = _rt(torch.randn(9000, 640, generator=g, device=cuda), dtype)
    q = _rt(torch.randn(9000, 384, generator=g, device=cuda), dtype)
    got = ops.concat_c(p, q)
    print(f"concat_c {dtype} 9000x(640+384): bit-identical = {torch.equal(got, torch.cat([p, q], -1))}")
    assert torch.equal(got, torch.cat([p, q], -1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layout_converters(cuda, dtype):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(9)
    src = torch.randn(2, 5, 33, 47, generator=g, device=cuda)
    for scale in (1.0, 0.18215):
        got = ops.nchw_to_nhwc(src, dtype, scale=scale)
        want = torch.zeros(2, 33, 47, 8, device=cuda, dtype=dtype)
        want[..., :5] = (src * scale).permute(0, 2, 3, 1).to(dtype)
        print(f"nchw_to_nhwc {dtype} scale {scale}: bit-identical = {torch.equal(got, want)}")
        assert torch.equal(got, want)
    # into a window of an existing tensor (c_off), the rest untouched
    out = torch.full((2, 33, 47, 16), 3.0, device=cuda, dtype=dtype)
    ops.nchw_to_nhwc(src, dtype, c_off=6, out=out)
    want = torch.full_like(out, 3.0)
    want[..., 6:11] = src.permute(0, 2, 3, 1).to(dtype)
    assert torch.equal(out, want)
    nhwc = _rt(torch.randn(2, 33, 47, 24, generator=g, device=cuda), dtype)
    got = ops.nhwc_to_nchw(nhwc, channels=5, c_off=8)
    want = nhwc[..., 8:13].permute(0, 3, 1, 2).float()
    print(f"nhwc_to_nchw {dtype}: bit-identical = {torch.equal(got, want)}")
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------- linear_small: ragged sizes, every activation pair
@pytest.mark.parametrize("act_in,act_out", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("rows,in_f,out_f,bias", [(3, 70, 13, True), (257, 323, 6, False), (1, 1, 1, True), (5, 1280, 7, True)])
def test_linear_small_ragged(cuda, act_in, act_out, rows, in_f, out_f, bias):
    from rsvld_amd import ops
    g = torch.Generator(device=cuda).manual_seed(rows * 1000 + in_f)
    x = torch.randn(rows, in_f, generator=g, device=cuda) * 2
    w = torch.randn(out_f, in_f, generator=g, device=cuda) / math.sqrt(in_f)
    b = torch.randn(out_f, generator=g, device=cuda) if bias else None
    got = ops.linear_small(x, w, b, act_in, act_out)
    xd = x.double()
    xa = xd * torch.sigmoid(xd) if act_in else xd
    pre = xa @ w.double().t() + (b.double() if bias else 0)
    ref = pre * torch.sigmoid(pre) if act_out else pre
    mag = xa.abs() @ w.double().abs().t() + (b.double().abs() if bias else 0)
    bound = (in_f / 64 + 10) * EPS32 * mag + 1e-30
    _check(f"linear_small {rows}x{in_f}->{out_f} bias={bias} act {act_in}{act_out}", got, ref, bound)
    assert _rejects(ref + (b.double() if bias else 0.5 * mag.clamp_min(1e-3)), ref, bound)   # bias added twice / missing


# ----------------------------------------------------------------------------- views: supported ones read in place, others refused
def test_supported_views_match_contiguous_copies(cuda):
    """Token-stride q | k | v slices of one fused tensor (attention) and channel-slice modulation (group_norm) must give results
    bit-identical to the same call on contiguous copies; an unsupported view raises before any launch.  Every view lies inside a
    larger contiguous buffer."""
    from rsvld_amd import _lib as L, ops
    g = torch.Generator(device=cuda).manual_seed(1)
    for heads, D, N in ((5, 64, 300), (1, 512, 200)):
        HD = heads * D
        qkv = torch.randn(2, N, 3 * HD, generator=g, device=cuda).half()
        q, k, v = qkv[..., :HD], qkv[..., HD:2 * HD], qkv[..., 2 * HD:]
        got = ops.attention(q, k, v, heads)
        want = ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), heads)
        print(f"attention heads={heads} D={D}: views bit-identical = {torch.equal(got, want)}")
        assert torch.equal(got, want)
        with pytest.raises(L.RsvldOperandError):            # inner stride 2: refused before launch
            wide = torch.zeros(2, N, 2 * HD, device=cuda, dtype=torch.float16)
            ops.attention(q, wide[..., ::2], v, heads)
    x = torch.randn(2, 8, 12, 64, generator=g, device=cuda).half()
    gb = torch.randn(2, 8, 12, 128, generator=g, device=cuda).half() * 0.1
    gamma, beta = torch.randn(64, generator=g, device=cuda), torch.randn(64, generator=g, device=cuda)
    got = ops.group_norm(x, gamma, beta, 32, 1e-5, mod_scale1p=gb[..., :64], mod_shift=gb[..., 64:])
    want = ops.group_norm(x, gamma, beta, 32, 1e-5, mod_scale1p=gb[..., :64].contiguous(), mod_shift=gb[..., 64:].contiguous())
    print(f"group_norm channel-slice modulation: bit-identical = {torch.equal(got, want)}")
    assert torch.equal(got, want)
    with pytest.raises(L.RsvldOperandError):                # a modulation tensor of another row stride than its partner
        ops.group_norm(x, gamma, beta, 32, 1e-5, mod_scale1p=gb[..., :64], mod_shift=gb[..., 64:].contiguous())
