// image.hip — the 8-bit image steps either side of the two diffusion stages: Pillow's 8-bit bicubic resize, the uint8 <-> fp32
// converters and ATen's fp32 bicubic fused with the 8-bit quantiser.  Every number that decides a bit (filter coefficients, bounds,
// look-up tables, tap indices) is built on the host (rsvld_amd/imageops.py) and arrives as a small device table; the kernels only
// gather, multiply-accumulate and store.  All of them are HBM-bound gathers.
#include "rsvld_common.h"

// hipcc contracts a * b + c into an FMA by default -- through __fmul_rn / __fadd_rn too, which are plain operators defined in a
// header that this pragma does not reach.  The quantisers and the fp32 bicubic must round every product and sum on its own, as torch and numpy do: one truncation boundary of Tensor2PIL per few thousand
// moves by a byte otherwise (tests/test_gpu_image.py::test_quantiser_edge_values_equal_the_host_functions).
#pragma clang fp contract(off)

namespace {

// One table row of Pillow's precompute_coeffs: taps [xmin, xmin + n) of the source axis.  Clamped against the axis length and the row
// width of the coefficient table, so that no table content can make a lane read outside its operands.
struct Taps { int lo, n; };
__device__ __forceinline__ Taps taps_of(const int32_t* __restrict__ bounds, int row, int in_len, int ksize) {
    int lo = bounds[2 * row], n = bounds[2 * row + 1];
    lo = min(max(lo, 0), in_len);
    n = min(min(max(n, 0), ksize), in_len - lo);
    return {lo, n};
}
// ImagingResampleHorizontal_8bpc / Vertical_8bpc: acc starts at 1 << (PRECISION_BITS - 1), clip8 = clamp(acc >> 22, 0, 255)
__device__ __forceinline__ uint8_t clip8(int32_t acc) { return (uint8_t)min(max(acc >> 22, 0), 255); }

// horizontal pass: dst[y][j][c] = clip8(sum_i src[y][xmin + i][c] * k[first + j][i]); one thread per output byte
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                         int in_w, int C, int out_len, int first, int ksize) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;       // byte of the output row
    if (b >= out_len * C) return;
    const int y = blockIdx.y, j = b / C, c = b - j * C;
    const Taps t = taps_of(bounds, first + j, in_w, ksize);
    const int32_t* k = coeffs + (int64_t)(first + j) * ksize;
    const uint8_t* s = src + ((int64_t)y * in_w + t.lo) * C + c;
    int32_t acc = 1 << 21;
    for (int i = 0; i < t.n; ++i) acc += (int32_t)s[(int64_t)i * C] * k[i];
    dst[(int64_t)y * out_len * C + b] = clip8(acc);
}

// vertical pass: elementwise over the bytes of a row.  VEC: 16 bytes per thread (row pitch and both bases whole 16-byte units)
template <bool VEC>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                         int in_h, int64_t pitch, int first, int ksize) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 16 : 1);
    if (b >= pitch) return;
    const int j = blockIdx.y;
    const Taps t = taps_of(bounds, first + j, in_h, ksize);
    const int32_t* k = coeffs + (int64_t)(first + j) * ksize;
    const uint8_t* s = src + (int64_t)t.lo * pitch + b;
    if (VEC) {
        int32_t acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 1 << 21;
        for (int i = 0; i < t.n; ++i) {
            const u32x4 v = *(const u32x4*)(s + (int64_t)i * pitch);
            const int32_t w = k[i];
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += (int32_t)((v[e >> 2] >> (8 * (e & 3))) & 0xffu) * w;
        }
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = (uint32_t)clip8(acc[4 * q]) | ((uint32_t)clip8(acc[4 * q + 1]) << 8) |
                   ((uint32_t)clip8(acc[4 * q + 2]) << 16) | ((uint32_t)clip8(acc[4 * q + 3]) << 24);
        *(u32x4*)(dst + (int64_t)j * pitch + b) = o;
    } else {
        int32_t acc = 1 << 21;
        for (int i = 0; i < t.n; ++i) acc += (int32_t)s[(int64_t)i * pitch] * k[i];
        dst[(int64_t)j * pitch + b] = clip8(acc);
    }
}

// uint8 HWC -> fp32 NCHW through a 256-entry table; one thread per pixel, the planes are written contiguously in W
__global__ __launch_bounds__(256) void u8_to_nchw_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                         float* __restrict__ dst, int64_t HW, int C) {
    __shared__ float tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    for (int c = 0; c < C; ++c) dst[c * HW + p] = tab[src[p * C + c]];
}

// The two 8-bit quantisers.  Every product and sum is rounded on its own (no contraction into an FMA: the pragma above), as torch
// and numpy evaluate the host expressions.  A NaN quantises to 0.
//   mode 0, tensor2img(min_max=(-1, 1)):  c = clamp(x, -1, 1); u = (c + 1) * 0.5; rint(u * 255), ties to even
//   mode 1, Tensor2PIL:                   t = x * 127.5 + 127.5; clamp to [0, 255]; truncate
__device__ __forceinline__ uint8_t quant8(float x, int mode) {
    if (x != x) return 0;
    if (mode == 0) {
        const float c = fminf(fmaxf(x, -1.f), 1.f);
        const float u = (c + 1.f) * 0.5f;
        return (uint8_t)(int)rintf(u * 255.f);
    }
    const float t = x * 127.5f + 127.5f;
    return (uint8_t)(int)fminf(fmaxf(t, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void nchw_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t HW,
                                                         int C, int mode) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    for (int c = 0; c < C; ++c) dst[p * C + c] = quant8(src[c * HW + p], mode);
}

// ATen's upsample_bicubic2d (align_corners = False) of an fp32 NCHW image, quantised as Tensor2PIL: per axis 4 clamped tap indices
// and 4 fp32 weights per output position; rows first (x taps), then the 4 row values with the y weights, each sum left to right.
__global__ __launch_bounds__(256) void bicubic_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const int32_t* __restrict__ iy, const float* __restrict__ wy,
                                                            const int32_t* __restrict__ ix, const float* __restrict__ wx, int C,
                                                            int H, int W, int w0) {
    const int ox = blockIdx.x * blockDim.x + threadIdx.x;
    if (ox >= w0) return;
    const int oy = blockIdx.y;
    int xs[4], ys[4];
    float kx[4], ky[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xs[i] = min(max(ix[4 * ox + i], 0), W - 1);
        ys[i] = min(max(iy[4 * oy + i], 0), H - 1);
        kx[i] = wx[4 * ox + i];
        ky[i] = wy[4 * oy + i];
    }
    for (int c = 0; c < C; ++c) {
        const float* plane = src + (int64_t)c * H * W;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* r = plane + (int64_t)ys[i] * W;
            float t = kx[0] * r[xs[0]];
#pragma unroll
            for (int j = 1; j < 4; ++j) t = t + kx[j] * r[xs[j]];
            v = i == 0 ? ky[0] * t : v + ky[i] * t;
        }
        dst[((int64_t)oy * w0 + ox) * C + c] = quant8(v, 1);
    }
}

// The caption's anyres views (llava_next.process_anyres_image after its two resizes): view 0 is the squashed image, view 1 + ty gx + tx
// the S x S tile (tx, ty) of a black canvas on which `fit` sits at (ox, oy); every byte goes through the table of its channel.  One
// thread per output pixel, the three planes written contiguously in x.  E carries the BITS of the output type (the table holds values of
// that type already), so fp16 and bf16 are one instantiation; the table and the output arrive untyped, so that both instantiations are
// one function type and one launch site.  A canvas pixel outside the pasted rectangle is byte 0, i.e. lut[c][0];
// the rectangle test is also what keeps every read inside `fit`, and p < S * S what keeps it inside `whole`.
template <typename E>
__global__ __launch_bounds__(256) void clip_views_kernel(const uint8_t* __restrict__ whole, const uint8_t* __restrict__ fit,
                                                         const void* __restrict__ lut, void* __restrict__ dst, int S, int nw, int nh,
                                                         int ox, int oy, int gx, int64_t pixels) {
    __shared__ E tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = ((const E*)lut)[i];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // pixel of [view][y][x]
    if (g >= pixels) return;
    const int64_t SS = (int64_t)S * S;
    const int v = (int)(g / SS);
    const int p = (int)(g - v * SS);
    const uint8_t* s = nullptr;
    if (v == 0) {
        s = whole + (int64_t)p * 3;
    } else {
        const int y = p / S, x = p - y * S;
        const int ty = (v - 1) / gx, tx = (v - 1) - ty * gx;
        const int X = tx * S + x - ox, Y = ty * S + y - oy;
        if (X >= 0 && X < nw && Y >= 0 && Y < nh) s = fit + ((int64_t)Y * nw + X) * 3;
    }
    E* d = (E*)dst + (int64_t)v * 3 * SS + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * SS] = tab[c * 256 + (s ? s[c] : 0)];
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int rsvld_resample_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* coeffs, int in_h,
                                 int in_w, int channels, int axis, int out_len, int first, int table_len, int ksize,
                                 void* stream) {
    if (!src || !dst || !bounds || !coeffs || in_h <= 0 || in_w <= 0 || channels <= 0 || channels > 4 || out_len <= 0 ||
        first < 0 || (int64_t)first + out_len > table_len || ksize <= 0 || (axis != 0 && axis != 1))
        return RSVLD_EINVAL;
    if ((int64_t)in_h * in_w * channels > INT32_MAX || (int64_t)out_len * (axis == 0 ? in_h : in_w) * channels > INT32_MAX)
        return RSVLD_EINVAL;
    if ((axis == 0 ? in_h : out_len) > 65535) return RSVLD_EUNSUPPORTED;      // rows ride on gridDim.y
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0) {
        hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((out_len * channels + 255) / 256), (unsigned)in_h), dim3(256), 0, s,
                           src, dst, bounds, coeffs, in_w, channels, out_len, first, ksize);
    } else {
        const int64_t pitch = (int64_t)in_w * channels;
        const bool vec = pitch % 16 == 0 && aligned16(src) && aligned16(dst);
        const auto kern = vec ? resample_v_kernel<true> : resample_v_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)cdiv64(vec ? pitch / 16 : pitch, 256), (unsigned)out_len), dim3(256), 0, s, src, dst,
                           bounds, coeffs, in_h, pitch, first, ksize);
    }
    return rsvld_check_launch();
}

extern "C" int rsvld_u8_hwc_to_nchw_f32(const uint8_t* src, const float* lut, float* dst, int H, int W, int channels,
                                        void* stream) {
    if (!src || !lut || !dst || H <= 0 || W <= 0 || channels <= 0 || channels > 4) return RSVLD_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(u8_to_nchw_kernel, dim3((unsigned)cdiv64(HW, 256)), dim3(256), 0, (hipStream_t)stream, src, lut, dst, HW,
                       channels);
    return rsvld_check_launch();
}

extern "C" int rsvld_nchw_f32_to_u8_hwc(const float* src, uint8_t* dst, int H, int W, int channels, int mode, void* stream) {
    if (!src || !dst || H <= 0 || W <= 0 || channels <= 0 || channels > 4 || (mode != 0 && mode != 1)) return RSVLD_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(nchw_to_u8_kernel, dim3((unsigned)cdiv64(HW, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, HW,
                       channels, mode);
    return rsvld_check_launch();
}

extern "C" int rsvld_bicubic_f32_to_u8_hwc(const float* src, uint8_t* dst, const int32_t* idx_y, const float* w_y,
                                           const int32_t* idx_x, const float* w_x, int channels, int H, int W, int h0, int w0,
                                           void* stream) {
    if (!src || !dst || !idx_y || !w_y || !idx_x || !w_x || channels <= 0 || channels > 4 || H <= 0 || W <= 0 || h0 <= 0 ||
        w0 <= 0)
        return RSVLD_EINVAL;
    if (h0 > 65535) return RSVLD_EUNSUPPORTED;                                // rows ride on gridDim.y
    hipLaunchKernelGGL(bicubic_to_u8_kernel, dim3((unsigned)((w0 + 255) / 256), (unsigned)h0), dim3(256), 0, (hipStream_t)stream,
                       src, dst, idx_y, w_y, idx_x, w_x, channels, H, W, w0);
    return rsvld_check_launch();
}

extern "C" int rsvld_clip_views_u8(const uint8_t* whole, const uint8_t* fit, const void* lut, void* dst, int S, int nw, int nh,
                                   int ox, int oy, int gx, int gy, int dtype, void* stream) {
    if (!whole || !fit || !lut || !dst || S <= 0 || nw <= 0 || nh <= 0 || ox < 0 || oy < 0 || gx <= 0 || gy <= 0) return RSVLD_EINVAL;
    if ((int64_t)ox + nw > (int64_t)gx * S || (int64_t)oy + nh > (int64_t)gy * S) return RSVLD_EINVAL;      // the paste leaves the canvas
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16 && dtype != RSVLD_F32) return RSVLD_EUNSUPPORTED;
    if (S > 32768 || gx > 32768 || gy > 32768 || (int64_t)gx * S > INT32_MAX / 4 || (int64_t)gy * S > INT32_MAX / 4)
        return RSVLD_EUNSUPPORTED;
    const int64_t pixels = (1 + (int64_t)gx * gy) * S * S;
    if (pixels * 3 > INT32_MAX) return RSVLD_EUNSUPPORTED;                    // (also: the workgroups ride on gridDim.x)
    const dim3 grid((unsigned)cdiv64(pixels, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const auto kern = dtype == RSVLD_F32 ? clip_views_kernel<uint32_t> : clip_views_kernel<uint16_t>;
    hipLaunchKernelGGL(kern, grid, block, 0, s, whole, fit, lut, dst, S, nw, nh, ox, oy, gx, pixels);
    return rsvld_check_launch();
}
