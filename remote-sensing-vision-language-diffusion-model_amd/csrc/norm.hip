// norm.hip — GroupNorm (+SiLU, +ZeroSFT modulation) and LayerNorm over NHWC / token-major tensors, for both the 16-bit
// networks (f16 / bf16 in and out) and the fp32-input networks of the "split" precision (round 4; RSVLD_SPLIT): there the residual
// stream is fp32 NHWC, and every tensor that only feeds a matrix product leaves its producer as two bf16 planes per row,
// [lo(C) | hi(C)] with hi = bf16(v), lo = bf16(v - hi).  The two families share the partial pass (one template over an input
// trait), the geometry, the source selection, the reduction tails, the output-form store and the host side; the apply pass and
// LayerNorm stay one kernel per family (see there).
// HBM-bound: every pass moves 16 B (fp32 input: 32 B) per lane and row.  Statistics: per-block partials merged in fp64 in a fixed
// order (deterministic, no atomics); an fp32 input's partials are fp64 themselves, from pivoted fp32 sums: see "pivot sums" below.
#include "rsvld_common.h"
#include "rsvld_plan.h"
#include <cstdint>
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------------------
// input/output traits: element types, the in-register raw piece of 8 channels, load, cvt to 8 floats, store of 8 channels
// at channel c of row `row`, U, the rows a GroupNorm thread keeps in flight, and LayerNorm's rows per wave and block cap
// ---------------------------------------------------------------------------------------
template <typename T>
struct Io16 {   // f16 / bf16 rows in and out: 16 B per piece
    typedef T in;
    typedef T out;
    typedef u32x4 raw;
    static constexpr int U = 4;   // 4 independent 16-B loads in flight
    static constexpr bool PIVOT = false;   // plain fp32 sums inside a thread (see "pivot sums")
    typedef float part;                    // ... and fp32 row-chunk partials: this pass is what it always was
    static constexpr int ln_rows(int maxc) { return maxc <= 2 ? 4 : maxc == 3 ? 3 : maxc == 4 ? 2 : 1; }   // LayerNorm rows per wave
    // at most 4096 blocks: waves keep gamma / beta in registers over their rows
    static constexpr int LN_MAX_BLOCKS = 4096;
    static __device__ __forceinline__ void load(const T* p, raw& r) { r = *(const u32x4*)p; }
    static __device__ __forceinline__ void cvt(const raw& r, float (&f)[8]) { unpack8<T>(r, f); }
    static __device__ __forceinline__ void store(T* y, int64_t row, int C, int c, const float (&f)[8]) {
        *(u32x4*)(y + row * C + c) = pack8<T>(f);
    }
};

// the output forms of the fp32-input entry points (their `out_f32` argument)
enum { OUT_PLANES = 0, OUT_F32 = 1, OUT_F16 = 2, OUT_HQ8 = 3 };   // bf16 planes, fp32, fp16, RSVLD_F16Q8 rows

// planes row: lo at [c], hi at [C + c].  (split8 of rsvld_common.h in this file's own words: built on split8 the same values
// come out, but gn_apply_split_kernel<planes> reorders its conversions, same instruction count)
__device__ __forceinline__ void st_planes8(bf16* row, int C, int c, const float (&f)[8]) {
    bf16x8 hv;
    float lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { hv[e] = (bf16)f[e]; lo[e] = f[e] - (float)hv[e]; }
    *(u32x4*)(row + c) = pack8<bf16>(lo);
    *(u32x4*)(row + C + c) = __builtin_bit_cast(u32x4, hv);
}
template <int OUT>
struct IoF32 {   // fp32 rows in (32 B per piece), OUT rows out
    typedef float in;
    typedef void out;
    typedef float raw[8];
    static constexpr int out_form = OUT;
    static constexpr int U = 2;   // two rows (4 x 16 B) in flight
    static constexpr bool PIVOT = true;
    typedef double part;
    static constexpr int ln_rows(int maxc) { return maxc <= 3 ? 2 : 1; }
    // at most ~3 resident workgroups per CU of a 256-CU chip: a wave then walks several row groups and its gamma / beta rows (as many
    // bytes as two rows of x at C = 1 280) are loaded once per wave instead of once per two rows (round 5: 4 096 workgroups of one row
    // group each ran the 32 768 x 1 280 LayerNorms of Stage 2 at 2.5 TB/s)
    static constexpr int LN_MAX_BLOCKS = 768;
    static __device__ __forceinline__ void load(const float* p, raw& r) { ld8f(p, r); }
    static __device__ __forceinline__ void cvt(const raw& r, float (&f)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = r[e];
    }
    static __device__ __forceinline__ void store(void* y, int64_t row, int C, int c, const float (&f)[8]) {
        if (OUT == OUT_F32) st8f((float*)y + row * C + c, f);
        else if (OUT == OUT_F16) *(u32x4*)((f16*)y + row * C + c) = pack8<f16>(f);
        else if (OUT == OUT_HQ8) st_hq8<true, RSVLD_HQ8_SX_LO, RSVLD_HQ8_SX_HI>((f16*)y + row * (2 * (int64_t)C), C, c, f);
        else st_planes8((bf16*)y + row * (2 * (int64_t)C), C, c, f);
    }
};
typedef IoF32<OUT_F32> InF32;   // for the passes that only read

// ---------------------------------------------------------------------------------------
// chunk geometry of the row-streaming GroupNorm passes (host and device): a thread owns the 8-channel chunks tc, tc + TPR, ...
// of the rows rsub, rsub + rif, ... of its block
// ---------------------------------------------------------------------------------------
struct GnGeom {
    int C, C8, C1_8;
    int TPR;   // threads per row
    int rif;   // rows in flight
    __host__ __device__ GnGeom(int C1, int C2) {
        C = C1 + C2, C8 = C >> 3, C1_8 = C1 >> 3;
        TPR = rsvld_plan::gn_threads_per_row(C8);
        rif = 256 / TPR;
    }
    // gn_partial_kernel's [rif][C][2], and the pivots [C] where it has them
    size_t lds_bytes(bool pivots) const { return ((size_t)rif * C * 2 + (pivots ? C : 0)) * sizeof(float); }
};

// chunk cc of image b of the channel concatenation [x1 (C1) | x2 (C2)]: declares src (its source's first row), cstride (that
// source's row stride) and coff (the chunk's channel offset there).  A macro: as a function or a small struct it reorders
// gn_partial_kernel's selects.
#define GN_SOURCE(T, x1, x2, b, HW, C1, C2, C1_8, cc)                                           \
    const T* src;                                                                               \
    int64_t cstride;                                                                            \
    int coff;                                                                                   \
    if (cc < C1_8) { src = x1 + (int64_t)b * HW * C1; cstride = C1; coff = cc * 8; }            \
    else { src = x2 + (int64_t)b * HW * C2; cstride = C2; coff = (cc - C1_8) * 8; }

// ---------------------------------------------------------------------------------------
// reduction tails, one copy each
// ---------------------------------------------------------------------------------------
// Sums of s and ss (doubles) over the 256 threads of a block: GN_BLOCK_PUT2 in every thread (wave shuffles, then the four wave
// partials into red[2][4] in LDS, and a barrier), GN_BLOCK_GET2 in the one thread that goes on with the sums (a fixed order).
// Macros: as a function (sums by reference or by value, red passed or declared inside, thread 0's part as a continuation, a second
// helper or an `if` of its own) the block reduction reorders gn_ab_kernel and adds a line to every gn_small_kernel.
#define GN_WAVE_SUM2(s, ss) \
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
#define GN_BLOCK_PUT2(s, ss, red, tid)                                                \
    GN_WAVE_SUM2(s, ss)                                                               \
    if (((tid) & 63) == 0) { red[0][(tid) >> 6] = s; red[1][(tid) >> 6] = ss; }       \
    __syncthreads()
#define GN_BLOCK_GET2(s, ss, red)                                \
    s = red[0][0] + red[0][1] + red[0][2] + red[0][3];           \
    ss = red[1][0] + red[1][1] + red[1][2] + red[1][3]
// Pivot sums.  var = E[x^2] - mean^2 from (sum, sumsq) needs the pair to 2^-p (mean / sigma)^2 of the variance: fp64 holds that for any
// input these kernels can store, fp32 does not (2^-24 * 64^2 = 2.4e-4 of the variance at mean / sigma = 64).  So every (sum, sumsq) of an
// fp32 tensor that leaves a block is fp64.  Inside a thread the sums stay fp32 and cheap: the thread subtracts a pivot k -- one of
// the very values it sums, so |x - k| is a few sigma -- and keeps s = sum (x - k), q = sum (x - k)^2, which carry the spread alone; then
// (sum, sumsq) = (s + n k, q + 2 k s + n k^2) in fp64.  One subtraction per element, no further pass over the data, and exact
// integer sums where the old fp32 pair was exact.
// The fp32-input kernels do this.  The 16-bit kernels (the row-chunk pass with its fp32 partials, and the one-workgroup kernel) are
// unchanged, so their statistics are bit for bit what they were: there the subtraction costs time (+3.4 % on a 1024 x 1024 x 64
// map) and buys nothing the 16-bit bounds can see -- the storage types stop at mean / sigma = 128 (fp16) and 16 (bf16), where the
// fp32 pair leaves 2.4e-3 and 6e-5 of the variance.
__device__ __forceinline__ void gn_unpivot(double s, double q, double n, double k, double& sum, double& sumsq) {
    sum = s + n * k;
    sumsq = q + k * (2.0 * s + n * k);
}
// fp64 sums -> mean and biased variance, clamped at 0
__device__ __forceinline__ void gn_moments(double s, double ss, double inv_count, double& mean, double& var) {
    mean = s * inv_count;
    var = ss * inv_count - mean * mean;
    if (var < 0.0) var = 0.0;
}
// per-channel affine (a, s) = (gamma rstd, beta - mean gamma rstd).  gn_apply_kernel forms a = gamma / sqrtf(var + eps), every
// other site a = gamma * (1 / sqrtf(var + eps)); the two round differently and both stay.  (The scale term as a function
// reorders gn_small_kernel<T, false>: two macros.)
#define GN_AFFINE_A_MUL(gamma, c, rstd) ((gamma ? gamma[c] : 1.f) * (rstd))
#define GN_AFFINE_A_DIV(gamma, c, sd) ((gamma ? gamma[c] : 1.f) / (sd))
__device__ __forceinline__ float gn_affine_s(const float* beta, int c, float mean, float a) { return (beta ? beta[c] : 0.f) - mean * a; }

// ---------------------------------------------------------------------------------------
// pass 1: per (image, row-chunk) partial sums  part[b][chunk][g] = (sum, sumsq), fp64 for an fp32 input (In::part)
// thread -> fixed 8-channel chunk, strided over rows; per-channel sums go through LDS so
// that any group size (2 .. C/groups, not necessarily a multiple of 8) is handled.
// A channel's pivot is its value in the chunk's first row, for every thread of the block (kept in LDS for the threads that add
// the groups up), so the LDS rows stay fp32 pairs of pivoted sums.
// ---------------------------------------------------------------------------------------
template <typename In>
__global__ __launch_bounds__(256) void gn_partial_kernel(const typename In::in* __restrict__ x1,
                                                         const typename In::in* __restrict__ x2, typename In::part* __restrict__ part,
                                                         int HW, int C1, int C2, int groups, int rows_per_chunk, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = (float*)smem_raw;  // [rif][C][2]
    const GnGeom geo(C1, C2);
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int row_lo = chunk * rows_per_chunk;
    const int row_hi = min(HW, row_lo + rows_per_chunk);
    const int tc = tid % geo.TPR, rsub = tid / geo.TPR;
    if (rsub < geo.rif) {
        for (int cc = tc; cc < geo.C8; cc += geo.TPR) {
            float s[8], ss[8], k[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { s[e] = 0.f; ss[e] = 0.f; }
            GN_SOURCE(typename In::in, x1, x2, b, HW, C1, C2, geo.C1_8, cc)
            if constexpr (In::PIVOT) {
                typename In::raw v;
                In::load(src + (int64_t)row_lo * cstride + coff, v);
                In::cvt(v, k);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) k[e] = 0.f;
            }
            int r = row_lo + rsub;
            if constexpr (In::U == 2) {   // (fp32 input in its own words: through the generic loop below it compiles 13 lines shorter)
                for (; r + geo.rif < row_hi; r += 2 * geo.rif) {
                    float f0[8], f1[8];
                    ld8f(src + (int64_t)r * cstride + coff, f0);
                    ld8f(src + (int64_t)(r + geo.rif) * cstride + coff, f1);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = f0[e] - k[e]; s[e] += d; ss[e] += d * d; }
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = f1[e] - k[e]; s[e] += d; ss[e] += d * d; }
                }
            } else
            for (; r + (In::U - 1) * geo.rif < row_hi; r += In::U * geo.rif) {  // U independent rows in flight
                typename In::raw v[In::U];
#pragma unroll
                for (int u = 0; u < In::U; ++u) In::load(src + (int64_t)(r + u * geo.rif) * cstride + coff, v[u]);
#pragma unroll
                for (int u = 0; u < In::U; ++u) {
                    float f[8];
                    In::cvt(v[u], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = f[e] - k[e]; s[e] += d; ss[e] += d * d; }
                }
            }
            for (; r < row_hi; r += geo.rif) {
                typename In::raw v;
                In::load(src + (int64_t)r * cstride + coff, v);
                float f[8];
                In::cvt(v, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = f[e] - k[e]; s[e] += d; ss[e] += d * d; }
            }
            float* dst = sm + ((int64_t)rsub * geo.C + cc * 8) * 2;
#pragma unroll
            for (int e = 0; e < 8; ++e) { dst[2 * e] = s[e]; dst[2 * e + 1] = ss[e]; }
            if (In::PIVOT && rsub == 0) {   // (after the row loop: stored before it, the pivot's load would have to land before the first row is asked for)
#pragma unroll
                for (int e = 0; e < 8; ++e) sm[geo.rif * geo.C * 2 + cc * 8 + e] = k[e];
            }
        }
    }
    __syncthreads();
    const int gs = geo.C / groups;
    for (int g = tid; g < groups; g += 256) {
        typename In::part* o = part + (((int64_t)b * nchunks + chunk) * groups + g) * 2;
        if constexpr (In::PIVOT) {
            const double nrows = (double)(row_hi - row_lo);
            double s = 0.0, ss = 0.0;
            for (int e = 0; e < gs; ++e) {
                const int c = g * gs + e;
                float cs = 0.f, cq = 0.f;   // the channel's pivoted sums over the rows in flight
                for (int r = 0; r < geo.rif; ++r) {
                    const float* q = sm + ((int64_t)r * geo.C + c) * 2;
                    cs += q[0];
                    cq += q[1];
                }
                double sum, sumsq;
                gn_unpivot((double)cs, (double)cq, nrows, (double)sm[geo.rif * geo.C * 2 + c], sum, sumsq);
                s += sum;
                ss += sumsq;
            }
            o[0] = s;
            o[1] = ss;
        } else {
            float s = 0.f, ss = 0.f;
            for (int r = 0; r < geo.rif; ++r) {
                const float* src = sm + ((int64_t)r * geo.C + g * gs) * 2;
                for (int e = 0; e < gs; ++e) { s += src[2 * e]; ss += src[2 * e + 1]; }
            }
            o[0] = s;
            o[1] = ss;
        }
    }
}

// pass 2: stats[b][g] = (mean, biased var); one wave per (image, group), lanes stride over the
// chunk partials, fp64 merge in a fixed order (deterministic)
template <typename P>
__global__ __launch_bounds__(256) void gn_finalize_kernel(const P* __restrict__ part, float* __restrict__ stats,
                                                          int groups, int nchunks, double inv_count, int total) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= total) return;
    const int b = i / groups, g = i - b * groups;
    double s = 0.0, ss = 0.0;
    for (int c = lane; c < nchunks; c += 64) {
        const P* p = part + (((int64_t)b * nchunks + c) * groups + g) * 2;
        s += (double)p[0];
        ss += (double)p[1];
    }
    GN_WAVE_SUM2(s, ss)
    if (lane == 0) {
        double mean, var;
        gn_moments(s, ss, inv_count, mean, var);
        stats[2 * i] = (float)mean;
        stats[2 * i + 1] = (float)var;
    }
}

// One block per (image, group): merge partial sums in fp64 (fixed order -> deterministic) and emit the
// per-channel affine ab[b][c] = (gamma*rstd, beta - mean*gamma*rstd) of that group's channels.
//   PER_CHANNEL = false: partials [b][chunk][group][2] from gn_partial_kernel (a statistics pass over x)
//   PER_CHANNEL = true : partials [b][tile][Cset][2] written by a conv epilogue (conv_halo.hip), one or two
//                        producers (the skip concat [x | x2] is normalised jointly)
//   P: the partials' type: double from an epilogue or an fp32 input's statistics pass, float from a 16-bit input's
template <bool PER_CHANNEL, typename P>
__global__ __launch_bounds__(256) void gn_ab_kernel(const P* __restrict__ part1, int n1, int C1,
                                                    const P* __restrict__ part2, int n2, int C2,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ ab, float* __restrict__ stats_out, int groups,
                                                    float eps, double inv_count) {
    __shared__ double red[2][4];
    __shared__ float mr[2];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int C = C1 + C2, gs = C / groups;
    double s = 0.0, ss = 0.0;
    if (PER_CHANNEL) {
        for (int c = g * gs; c < (g + 1) * gs; ++c) {
            const P* base;
            int n, Cs, cc;
            if (c < C1) { base = part1 + (int64_t)b * n1 * C1 * 2; n = n1; Cs = C1; cc = c; }
            else { base = part2 + (int64_t)b * n2 * C2 * 2; n = n2; Cs = C2; cc = c - C1; }
            for (int t = tid; t < n; t += 256) {
                s += (double)base[((int64_t)t * Cs + cc) * 2];
                ss += (double)base[((int64_t)t * Cs + cc) * 2 + 1];
            }
        }
    } else {
        for (int t = tid; t < n1; t += 256) {
            const P* q = part1 + (((int64_t)b * n1 + t) * groups + g) * 2;
            s += (double)q[0];
            ss += (double)q[1];
        }
    }
    GN_BLOCK_PUT2(s, ss, red, tid);
    if (tid == 0) {
        GN_BLOCK_GET2(s, ss, red);
        double mean, var;
        gn_moments(s, ss, inv_count, mean, var);
        mr[0] = (float)mean;
        mr[1] = (float)var;
        if (stats_out != nullptr) {
            stats_out[((int64_t)b * groups + g) * 2] = (float)mean;
            stats_out[((int64_t)b * groups + g) * 2 + 1] = (float)var;
        }
    }
    __syncthreads();
    if (ab != nullptr) {
        const float mean = mr[0], rstd = 1.0f / sqrtf(mr[1] + eps);
        for (int c = g * gs + tid; c < (g + 1) * gs; c += 256) {
            const float a = GN_AFFINE_A_MUL(gamma, c, rstd);
            ab[((int64_t)b * C + c) * 2] = a;
            ab[((int64_t)b * C + c) * 2 + 1] = gn_affine_s(beta, c, mean, a);
        }
    }
}

// pass 3: y = act((x-mean)*rstd*gamma+beta) [*(1+scale1p)+shift]
// grid (row-chunks, B).  Same thread <-> channel-chunk mapping as pass 1: a thread keeps ONE
// 8-channel chunk, so its 8 (scale, shift) pairs live in registers and the row loop is pure
// 16-byte streaming with 4 loads in flight.
// The 16-bit and the fp32-input apply pass stay two kernels in their own words.  One kernel over both argument lists moves
// every instantiation's argument offsets; two kernels around a shared emit body and row loops (over the traits above, the
// preamble called back or kept in each kernel) move the 16-bit kernels by +58 .. +66 instruction lines and the four fp32-input
// ones by -74 .. +11.  They share the geometry, the source selection and the affine.
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x1, const T* __restrict__ x2,
                                                       T* __restrict__ y, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const T* __restrict__ mod_scale, const T* __restrict__ mod_shift,
                                                       int HW, int C1, int C2, int groups, float eps, int silu,
                                                       int rows_per_block, int mod_stride) {
    const GnGeom geo(C1, C2);
    const int tid = threadIdx.x;
    const int tc = tid % geo.TPR, rsub = tid / geo.TPR;
    if (rsub >= geo.rif) return;
    const int b = blockIdx.y;
    const int gs = geo.C / groups;
    const int row_lo = blockIdx.x * rows_per_block;
    const int row_hi = min(HW, row_lo + rows_per_block);
    for (int cc = tc; cc < geo.C8; cc += geo.TPR) {
        float sa[8], sb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = cc * 8 + e;
            const int g = ch / gs;
            const float mean = stats[((int64_t)b * groups + g) * 2];
            const float var = stats[((int64_t)b * groups + g) * 2 + 1];
            const float a = GN_AFFINE_A_DIV(gamma, ch, sqrtf(var + eps));
            sa[e] = a;
            sb[e] = gn_affine_s(beta, ch, mean, a);
        }
        GN_SOURCE(T, x1, x2, b, HW, C1, C2, geo.C1_8, cc)
        T* dst = y + (int64_t)b * HW * geo.C + cc * 8;
        auto emit = [&](int r, const u32x4& v) {
            float f[8];
            unpack8<T>(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float t = f[e] * sa[e] + sb[e];
                if (silu) t = silu_f(t);
                f[e] = t;
            }
            const int64_t o = (int64_t)r * geo.C;
            if (mod_scale != nullptr) {
                const int64_t mo = ((int64_t)b * HW + r) * mod_stride + cc * 8;
                float ms[8], mh[8];
                unpack8<T>(*(const u32x4*)(mod_scale + mo), ms);
                unpack8<T>(*(const u32x4*)(mod_shift + mo), mh);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = f[e] * (1.f + ms[e]) + mh[e];
            }
            *(u32x4*)(dst + o) = pack8<T>(f);
        };
        int r = row_lo + rsub;
        for (; r + 3 * geo.rif < row_hi; r += 4 * geo.rif) {
            u32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const u32x4*)(src + (int64_t)(r + u * geo.rif) * cstride + coff);
#pragma unroll
            for (int u = 0; u < 4; ++u) emit(r + u * geo.rif, v[u]);
        }
        for (; r < row_hi; r += geo.rif) emit(r, *(const u32x4*)(src + (int64_t)r * cstride + coff));
    }
}

// y = act(a[b,c] * v + s[b,c]) [* (1 + mod_scale) + mod_shift]; fp32 in (one or two sources), the pairs from a ready ab row, OUT rows out
template <int OUT>
__global__ __launch_bounds__(256) void gn_apply_split_kernel(const float* __restrict__ x1, const float* __restrict__ x2, void* __restrict__ y,
                                                             const float* __restrict__ ab, const float* __restrict__ mod_scale,
                                                             const float* __restrict__ mod_shift, int HW, int C1, int C2, int silu,
                                                             int rows_per_block, int mod_stride) {
    const GnGeom geo(C1, C2);
    const int tid = threadIdx.x, tc = tid % geo.TPR, rsub = tid / geo.TPR;
    if (rsub >= geo.rif) return;
    const int b = blockIdx.y;
    const int row_lo = blockIdx.x * rows_per_block, row_hi = min(HW, row_lo + rows_per_block);
    for (int cc = tc; cc < geo.C8; cc += geo.TPR) {
        float sa[8], sb[8];
        {
            const float* a = ab + ((int64_t)b * geo.C + cc * 8) * 2;
#pragma unroll
            for (int e = 0; e < 8; ++e) { sa[e] = a[2 * e]; sb[e] = a[2 * e + 1]; }
        }
        GN_SOURCE(float, x1, x2, b, HW, C1, C2, geo.C1_8, cc)
        auto emit = [&](int r, float (&f)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = f[e] * sa[e] + sb[e];
                f[e] = silu ? silu_f(t) : t;
            }
            if (mod_scale != nullptr) {
                const int64_t mo = ((int64_t)b * HW + r) * mod_stride + cc * 8;
                float ms[8], mh[8];
                ld8f(mod_scale + mo, ms);
                ld8f(mod_shift + mo, mh);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = f[e] * (1.f + ms[e]) + mh[e];
            }
            const int64_t pix = (int64_t)b * HW + r;
            // (planes: the row width as an int; through IoF32's store, which forms it in 64 bits, this kernel grows by 13 lines)
            if (OUT == OUT_PLANES) st_planes8((bf16*)y + pix * (2 * geo.C), geo.C, cc * 8, f);
            else IoF32<OUT>::store(y, pix, geo.C, cc * 8, f);
        };
        int r = row_lo + rsub;
        for (; r + geo.rif < row_hi; r += 2 * geo.rif) {
            float f0[8], f1[8];
            ld8f(src + (int64_t)r * cstride + coff, f0);
            ld8f(src + (int64_t)(r + geo.rif) * cstride + coff, f1);
            emit(r, f0);
            emit(r + geo.rif, f1);
        }
        for (; r < row_hi; r += geo.rif) {
            float f[8];
            ld8f(src + (int64_t)r * cstride + coff, f);
            emit(r, f);
        }
    }
}

// LayerNorm: one wave per row, ROWS rows per wave with all their loads issued up front (a single row per wave
// is one dependent load -> reduce -> store chain: measured 15 us for 10 MB); rows kept in registers (C <= 4096),
// exact two-pass variance.
template <typename T, int MAXC, int ROWS>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int C8 = C >> 3;
    // gamma / beta of this lane's chunks stay in registers for every row the wave processes (read per element inside
    // the row loop they doubled the L1 traffic of the kernel: 2.2 TB/s on the 168 MB token tensors of Stage 2)
    float ga[MAXC][8], be[MAXC][8];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int cc = lane + 64 * j;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ga[j][e] = (gamma != nullptr && cc < C8) ? gamma[cc * 8 + e] : 1.f;
            be[j][e] = (beta != nullptr && cc < C8) ? beta[cc * 8 + e] : 0.f;
        }
    }
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row0 = wave_id * ROWS; row0 < rows; row0 += nwaves * ROWS) {
        u32x4 raw[ROWS][MAXC];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                const int cc = lane + 64 * j;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (cc < C8 && row0 + r < rows) v = *(const u32x4*)(x + (row0 + r) * C + cc * 8);
                raw[r][j] = v;
            }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (row0 + r >= rows) break;
            float f[MAXC][8];
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                unpack8<T>(raw[r][j], f[j]);
                if (lane + 64 * j < C8) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) s += f[j][e];
                }
            }
            const float mean = wave_sum(s) / (float)C;
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                if (lane + 64 * j < C8) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = f[j][e] - mean; ss += d * d; }
                }
            }
            const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                const int cc = lane + 64 * j;
                if (cc < C8) {
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (f[j][e] - mean) * rstd * ga[j][e] + be[j][e];
                    *(u32x4*)(y + (row0 + r) * C + cc * 8) = pack8<T>(o);
                }
            }
        }
    }
}

// LayerNorm of fp32 rows -> OUT rows: the 16-bit kernel's structure (one wave per row group, rows and the lane's gamma / beta in
// registers, exact two-pass variance) with 32-byte pieces.  The two stay apart: they differ in how a row piece is held (packed
// u32x4 by value / 8 floats in place), and one kernel over a trait for that moves layernorm_kernel<T, 8, 1> (registers renamed) or
// layernorm_split_kernel<4, 1, fp32> (-10 lines) with the piece in place, and 8 of the 12 fp32-input kernels with it by value.
template <int MAXC, int ROWS, int OUT>
__global__ __launch_bounds__(256) void layernorm_split_kernel(const float* __restrict__ x, void* __restrict__ y,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int C8 = C >> 3;
    float ga[MAXC][8], be[MAXC][8];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int cc = lane + 64 * j;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ga[j][e] = (gamma != nullptr && cc < C8) ? gamma[cc * 8 + e] : 1.f;
            be[j][e] = (beta != nullptr && cc < C8) ? beta[cc * 8 + e] : 0.f;
        }
    }
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row0 = wave_id * ROWS; row0 < rows; row0 += nwaves * ROWS) {
        float f[ROWS][MAXC][8];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                const int cc = lane + 64 * j;
                if (cc < C8 && row0 + r < rows) ld8f(x + (row0 + r) * C + cc * 8, f[r][j]);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[r][j][e] = 0.f;
                }
            }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (row0 + r >= rows) break;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (lane + 64 * j < C8) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) s += f[r][j][e];
                }
            const float mean = wave_sum(s) / (float)C;
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (lane + 64 * j < C8) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = f[r][j][e] - mean; ss += d * d; }
                }
            const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                const int cc = lane + 64 * j;
                if (cc < C8) {
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (f[r][j][e] - mean) * rstd * ga[j][e] + be[j][e];
                    IoF32<OUT>::store(y, row0 + r, C, cc * 8, o);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Small tensors (deep UNet levels: 32x32 / 64x64 maps): the three launches above are latency-bound (3 x ~7 us for
// 4 MB).  One workgroup per (image, group) instead: the group's HW x (C/groups) slab is read ONCE into registers
// (<= 32 sixteen-byte vectors per thread), reduced in fp64 through LDS in a fixed order, and either normalised and
// written (APPLY) or turned into the per-channel (scale, shift) rows of the fused conv prologue (!APPLY).
// Needs 8 | C/groups (a vector never straddles groups) and, for [x | x2], groups that do not straddle the sources.
// ---------------------------------------------------------------------------------------
using rsvld_plan::GN_SMALL_MAXV;

template <typename T, bool APPLY>
__global__ __launch_bounds__(256) void gn_small_kernel(const T* __restrict__ x1, const T* __restrict__ x2, T* __restrict__ y,
                                                       float* __restrict__ ab, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int HW, int C1, int C2, int groups,
                                                       float eps, int silu) {
    __shared__ double red[2][4];
    __shared__ float mr[2];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int C = C1 + C2, gs = C / groups, gs8 = gs >> 3;   // gs8 is a power of two <= 256
    const int ch0 = g * gs;
    const T* src;
    int cs, coff;
    if (ch0 < C1) { src = x1 + (int64_t)b * HW * C1; cs = C1; coff = ch0; }
    else { src = x2 + (int64_t)b * HW * C2; cs = C2; coff = ch0 - C1; }
    const int chunk = tid & (gs8 - 1);           // fixed per thread: 256 is a multiple of gs8
    const int row0 = tid / gs8, rstep = 256 / gs8;
    const int nv = (HW - row0 + rstep - 1) / rstep;   // vectors of this thread (<= GN_SMALL_MAXV, may be <= 0)
    u32x4 v[GN_SMALL_MAXV];
#pragma unroll
    for (int i = 0; i < GN_SMALL_MAXV; ++i)
        if (i < nv) v[i] = *(const u32x4*)(src + (int64_t)(row0 + i * rstep) * cs + coff + chunk * 8);
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int i = 0; i < GN_SMALL_MAXV; ++i)
        if (i < nv) {
            float f[8];
            unpack8<T>(v[i], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) { s += f[e]; ss += f[e] * f[e]; }
        }
    double ds = (double)s, dss = (double)ss;
    GN_BLOCK_PUT2(ds, dss, red, tid);
    if (tid == 0) {
        GN_BLOCK_GET2(ds, dss, red);
        const double inv_count = 1.0 / ((double)HW * (double)gs);
        double mean, var;
        gn_moments(ds, dss, inv_count, mean, var);
        mr[0] = (float)mean;
        mr[1] = (float)var;
    }
    __syncthreads();
    const float mean = mr[0], rstd = 1.0f / sqrtf(mr[1] + eps);
    if (!APPLY) {
        if (tid < gs) {
            const int c = ch0 + tid;
            const float a = GN_AFFINE_A_MUL(gamma, c, rstd);
            ab[((int64_t)b * C + c) * 2] = a;
            ab[((int64_t)b * C + c) * 2 + 1] = gn_affine_s(beta, c, mean, a);
        }
        return;
    }
    float sa[8], sb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch0 + chunk * 8 + e;
        sa[e] = GN_AFFINE_A_MUL(gamma, c, rstd);
        sb[e] = gn_affine_s(beta, c, mean, sa[e]);
    }
    T* dst = y + (int64_t)b * HW * C + ch0 + chunk * 8;
#pragma unroll
    for (int i = 0; i < GN_SMALL_MAXV; ++i)
        if (i < nv) {
            float f[8];
            unpack8<T>(v[i], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = f[e] * sa[e] + sb[e];
                f[e] = silu ? silu_f(t) : t;
            }
            *(u32x4*)(dst + (int64_t)(row0 + i * rstep) * C) = pack8<T>(f);
        }
}

// (mean, biased variance) per (image, group) -> the per-channel affine (gamma rstd, beta - mean gamma rstd)
__global__ void gn_ab_from_stats_kernel(const float* __restrict__ mean_var, const float* __restrict__ gamma, const float* __restrict__ beta,
                                        float* __restrict__ ab, int C, int groups, float eps, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (b, c)
    if (i >= total) return;
    const int b = i / C, c = i - b * C, g = c / (C / groups);
    const float mean = mean_var[((int64_t)b * groups + g) * 2], var = mean_var[((int64_t)b * groups + g) * 2 + 1];
    const float a = GN_AFFINE_A_MUL(gamma, c, 1.0f / sqrtf(var + eps));
    ab[2 * (int64_t)i] = a;
    ab[2 * (int64_t)i + 1] = gn_affine_s(beta, c, mean, a);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// which route, and the row chunks of the partials route: rsvld_plan.h
using rsvld_plan::GnPlan;
using rsvld_plan::gn_plan;
using rsvld_plan::gn_small_route;
using rsvld_plan::gn_dims_ok;
using rsvld_plan::gn_groups_ok;

// operand checks of the entry points: the sizes of [x (C1) | x2 (C2)] with its pointers (sizes and groups alone: rsvld_plan.h)
bool gn_x_ok(const void* x, const void* x2, int B, int HW, int C1, int C2) {
    return x != nullptr && gn_dims_ok(B, HW, C1, C2) && (C2 > 0) == (x2 != nullptr);
}
bool gn_align8(const void* p) { return ((uintptr_t)p & 7) == 0; }   // fp64 partials
bool gn_mod_ok(const void* mod_scale1p, const void* mod_shift, int mod_stride, int align) {
    return (mod_scale1p != nullptr) == (mod_shift != nullptr) && mod_stride >= 0 && mod_stride % align == 0;
}

double gn_inv_count(int HW, int C, int groups) { return 1.0 / ((double)HW * (double)(C / groups)); }

template <typename In>
bool launch_partials(const void* x, const void* x2, typename In::part* part, int B, int HW, int C1, int C2, int groups, const GnPlan& pl,
                     hipStream_t s) {
    typedef typename In::in T;
    const size_t lds = GnGeom(C1, C2).lds_bytes(In::PIVOT);
    // C > 5 460 with pivots: more than the 64 KiB of dynamic LDS a kernel gets unasked; registered once, with the maximum (C = 8192)
    if (lds > 65536 && rsvld_smem_once<gn_partial_kernel<In>>((int)GnGeom(8192, 0).lds_bytes(In::PIVOT)) != hipSuccess) return false;
    hipLaunchKernelGGL(gn_partial_kernel<In>, dim3(pl.nchunks, B), dim3(256), lds, s, (const T*)x,
                       (const T*)x2, part, HW, C1, C2, groups, pl.rows_per_chunk, pl.nchunks);
    return true;
}

// partials in ws -> (mean, var) rows
template <typename In>
int gn_stats_impl(const void* x, const void* x2, float* stats, int B, int HW, int C1, int C2, int groups, void* ws,
                  hipStream_t s) {
    const GnPlan pl = gn_plan(HW);
    typedef typename In::part P;
    if (!launch_partials<In>(x, x2, (P*)ws, B, HW, C1, C2, groups, pl, s)) return RSVLD_ELAUNCH;
    const int total = B * groups;
    hipLaunchKernelGGL(gn_finalize_kernel<P>, dim3((total + 3) / 4), dim3(256), 0, s, (const P*)ws, stats, groups, pl.nchunks,
                       gn_inv_count(HW, C1 + C2, groups), total);
    return rsvld_check_launch();
}

// partials in ws -> per-channel (scale, shift) rows
template <typename In>
int gn_scale_shift_impl(const void* x, const void* x2, const float* gamma, const float* beta, float* scale_shift, int B, int HW,
                        int C1, int C2, int groups, float eps, void* ws, hipStream_t s) {
    const GnPlan pl = gn_plan(HW);
    typedef typename In::part P;
    if (!launch_partials<In>(x, x2, (P*)ws, B, HW, C1, C2, groups, pl, s)) return RSVLD_ELAUNCH;
    hipLaunchKernelGGL((gn_ab_kernel<false, P>), dim3(groups, B), dim3(256), 0, s, (const P*)ws, pl.nchunks, C1 + C2, (const P*)nullptr, 0, 0,
                       gamma, beta, scale_shift, nullptr, groups, eps, gn_inv_count(HW, C1 + C2, groups));
    return rsvld_check_launch();
}

// the apply pass's rows per block and blocks per image: ~2048 blocks over the chip, at least U * rif rows per block so the
// unrolled loop is used
template <typename Io>
int gn_apply_rows_per_block(int B, int HW, int C1, int C2) {
    int max_blocks = 2048 / B;
    if (max_blocks < 1) max_blocks = 1;
    int rpb = (HW + max_blocks - 1) / max_blocks;
    const int min_rows = Io::U * GnGeom(C1, C2).rif;
    return rpb < min_rows ? min_rows : rpb;
}

template <typename T>
int gn_apply_impl(const void* x, const void* x2, void* y, const float* stats, const float* gamma, const float* beta,
                  const void* mscale, const void* mshift, int mod_stride, int B, int HW, int C1, int C2, int groups,
                  float eps, int silu, hipStream_t s) {
    const int rpb = gn_apply_rows_per_block<Io16<T>>(B, HW, C1, C2);
    hipLaunchKernelGGL(gn_apply_kernel<T>, dim3((unsigned)cdiv64(HW, rpb), B), dim3(256), 0, s, (const T*)x, (const T*)x2,
                       (T*)y, stats, gamma, beta, (const T*)mscale, (const T*)mshift, HW, C1, C2, groups, eps, silu,
                       rpb, mod_stride > 0 ? mod_stride : C1 + C2);
    return rsvld_check_launch();
}

template <typename T, bool APPLY>
int gn_small_impl(const void* x, const void* x2, void* y, float* ab, const float* gamma, const float* beta, int B, int HW, int C1,
                  int C2, int groups, float eps, int silu, hipStream_t s) {
    hipLaunchKernelGGL((gn_small_kernel<T, APPLY>), dim3(groups, B), dim3(256), 0, s, (const T*)x, (const T*)x2, (T*)y, ab, gamma,
                       beta, HW, C1, C2, groups, eps, silu);
    return rsvld_check_launch();
}

template <typename Io, int MAXC>
void launch_layernorm_maxc(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                           hipStream_t s) {
    constexpr int ROWS = Io::ln_rows(MAXC);   // rows per wave in flight; 4 waves per block
    const int64_t n = cdiv64(rows, 4 * ROWS);
    const dim3 grid((unsigned)(n < Io::LN_MAX_BLOCKS ? n : Io::LN_MAX_BLOCKS));
    if constexpr (std::is_same<typename Io::in, float>::value)
        hipLaunchKernelGGL((layernorm_split_kernel<MAXC, ROWS, Io::out_form>), grid, dim3(256), 0, s, (const float*)x, y, gamma, beta, rows, C, eps);
    else
        hipLaunchKernelGGL((layernorm_kernel<typename Io::in, MAXC, ROWS>), grid, dim3(256), 0, s, (const typename Io::in*)x, (typename Io::in*)y, gamma, beta, rows, C, eps);
}
template <typename Io>
void launch_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps, hipStream_t s) {
    const int chunks_per_lane = (C / 8 + 63) / 64;
    if (chunks_per_lane <= 2) launch_layernorm_maxc<Io, 2>(x, y, gamma, beta, rows, C, eps, s);         // C <= 1024
    else if (chunks_per_lane == 3) launch_layernorm_maxc<Io, 3>(x, y, gamma, beta, rows, C, eps, s);    // C <= 1536 (the 1280-channel transformer blocks)
    else if (chunks_per_lane <= 4) launch_layernorm_maxc<Io, 4>(x, y, gamma, beta, rows, C, eps, s);    // C <= 2048
    else launch_layernorm_maxc<Io, 8>(x, y, gamma, beta, rows, C, eps, s);
}

// f(IoF32<form>()) for an output form 0 .. MAX that the caller has range-checked
template <int MAX, typename F>
void with_out_form(int form, F f) {
    if constexpr (MAX >= OUT_HQ8) {
        if (form == OUT_HQ8) return f(IoF32<OUT_HQ8>());
    }
    if (form == OUT_F32) return f(IoF32<OUT_F32>());
    if (form == OUT_F16) return f(IoF32<OUT_F16>());
    return f(IoF32<OUT_PLANES>());
}

}  // namespace

extern "C" int rsvld_plan_groupnorm(int dtype, int B, int HW, int C1, int C2, int groups, rsvld_groupnorm_plan* plan) {
    return plan == nullptr ? RSVLD_EINVAL : rsvld_plan::plan_groupnorm(dtype, B, HW, C1, C2, groups, plan);
}

extern "C" int64_t rsvld_groupnorm_ws_bytes(int B, int HW, int C, int groups) {
    (void)C;
    if (B <= 0 || HW <= 0 || groups <= 0) return 0;
    const GnPlan pl = gn_plan(HW);
    // room for fp64 partials (an fp32 input's; a 16-bit input's are fp32 and fill half of it), then the final fp32 stats
    return (int64_t)B * pl.nchunks * groups * 2 * (int64_t)sizeof(double) + (int64_t)B * groups * 2 * (int64_t)sizeof(float);
}

extern "C" int rsvld_groupnorm_stats(const void* x, const void* x2, float* mean_var, int B, int HW, int C1, int C2,
                                     int groups, int dtype, void* ws, void* stream) {
    if (!mean_var || !ws || !gn_x_ok(x, x2, B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups)) return RSVLD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSVLD_F16) return gn_stats_impl<Io16<f16>>(x, x2, mean_var, B, HW, C1, C2, groups, ws, s);
    if (dtype == RSVLD_BF16) return gn_stats_impl<Io16<bf16>>(x, x2, mean_var, B, HW, C1, C2, groups, ws, s);
    return RSVLD_EINVAL;
}

extern "C" int rsvld_groupnorm_apply(const void* x, const void* x2, void* y, const float* mean_var,
                                     const float* gamma, const float* beta, const void* mod_scale1p,
                                     const void* mod_shift, int mod_stride, int B, int HW, int C1, int C2, int groups,
                                     float eps, int silu, int dtype, void* stream) {
    if (!y || !mean_var || !gn_x_ok(x, x2, B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups)) return RSVLD_EINVAL;
    if (!gn_mod_ok(mod_scale1p, mod_shift, mod_stride, 8)) return RSVLD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSVLD_F16)
        return gn_apply_impl<f16>(x, x2, y, mean_var, gamma, beta, mod_scale1p, mod_shift, mod_stride, B, HW, C1, C2, groups, eps, silu, s);
    if (dtype == RSVLD_BF16)
        return gn_apply_impl<bf16>(x, x2, y, mean_var, gamma, beta, mod_scale1p, mod_shift, mod_stride, B, HW, C1, C2, groups, eps, silu, s);
    return RSVLD_EINVAL;
}

extern "C" int rsvld_groupnorm_nhwc(const void* x, const void* x2, void* y, const float* gamma, const float* beta,
                                    const void* mod_scale1p, const void* mod_shift, int mod_stride, int B, int HW, int C1,
                                    int C2, int groups, float eps, int silu, int dtype, void* ws, void* stream) {
    if (!ws || !gn_dims_ok(B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups)) return RSVLD_EINVAL;
    if (mod_scale1p == nullptr && mod_shift == nullptr && y && gn_x_ok(x, x2, B, HW, C1, C2) &&
        gn_small_route(dtype, B, HW, C1, C2, groups)) {
        hipStream_t s = (hipStream_t)stream;
        if (dtype == RSVLD_F16) return gn_small_impl<f16, true>(x, x2, y, nullptr, gamma, beta, B, HW, C1, C2, groups, eps, silu, s);
        return gn_small_impl<bf16, true>(x, x2, y, nullptr, gamma, beta, B, HW, C1, C2, groups, eps, silu, s);
    }
    const GnPlan pl = gn_plan(HW);
    float* stats = (float*)((double*)ws + (int64_t)B * pl.nchunks * groups * 2);
    int rc = rsvld_groupnorm_stats(x, x2, stats, B, HW, C1, C2, groups, dtype, ws, stream);
    if (rc != RSVLD_OK) return rc;
    return rsvld_groupnorm_apply(x, x2, y, stats, gamma, beta, mod_scale1p, mod_shift, mod_stride, B, HW, C1, C2, groups,
                                 eps, silu, dtype, stream);
}

extern "C" int rsvld_groupnorm_scale_shift(const void* x, const void* x2, const float* gamma, const float* beta,
                                           float* scale_shift, int B, int HW, int C1, int C2, int groups, float eps,
                                           int dtype, void* ws, void* stream) {
    if (!ws || !scale_shift || !gn_x_ok(x, x2, B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups)) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (gn_small_route(dtype, B, HW, C1, C2, groups)) {
        if (dtype == RSVLD_F16) return gn_small_impl<f16, false>(x, x2, nullptr, scale_shift, gamma, beta, B, HW, C1, C2, groups, eps, 0, s);
        return gn_small_impl<bf16, false>(x, x2, nullptr, scale_shift, gamma, beta, B, HW, C1, C2, groups, eps, 0, s);
    }
    if (dtype == RSVLD_F16) return gn_scale_shift_impl<Io16<f16>>(x, x2, gamma, beta, scale_shift, B, HW, C1, C2, groups, eps, ws, s);
    return gn_scale_shift_impl<Io16<bf16>>(x, x2, gamma, beta, scale_shift, B, HW, C1, C2, groups, eps, ws, s);
}

extern "C" int rsvld_groupnorm_scale_shift_from_partials(const double* part1, int ntiles1, int C1, const double* part2,
                                                         int ntiles2, int C2, const float* gamma, const float* beta,
                                                         float* scale_shift, int B, int HW, int groups, float eps,
                                                         void* stream) {
    if (!part1 || !scale_shift || B <= 0 || HW <= 0 || C1 <= 0 || C2 < 0 || ntiles1 <= 0 || groups <= 0) return RSVLD_EINVAL;
    if ((C2 > 0) != (part2 != nullptr) || (C2 > 0 && ntiles2 <= 0) || (C1 + C2) % groups != 0 || B > 65535) return RSVLD_EINVAL;
    if (!gn_align8(part1) || !gn_align8(part2)) return RSVLD_EINVAL;
    hipLaunchKernelGGL((gn_ab_kernel<true, double>), dim3(groups, B), dim3(256), 0, (hipStream_t)stream, part1, ntiles1, C1, part2,
                       ntiles2, C2, gamma, beta, scale_shift, nullptr, groups, eps, gn_inv_count(HW, C1 + C2, groups));
    return rsvld_check_launch();
}

extern "C" int rsvld_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                               float eps, int dtype, void* stream) {
    if (!x || !y || rows <= 0 || C <= 0 || C % 8 || C > 4096) return RSVLD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSVLD_F16) launch_layernorm<Io16<f16>>(x, y, gamma, beta, rows, C, eps, s);
    else if (dtype == RSVLD_BF16) launch_layernorm<Io16<bf16>>(x, y, gamma, beta, rows, C, eps, s);
    else return RSVLD_EINVAL;
    return rsvld_check_launch();
}

// ---- split-operand product path (fp32 NHWC in)
extern "C" int rsvld_groupnorm_scale_shift_f32(const float* x, const float* x2, const float* gamma, const float* beta,
                                               float* scale_shift, int B, int HW, int C1, int C2, int groups, float eps, void* ws,
                                               void* stream) {
    if (!ws || !gn_align8(ws) || !scale_shift || !gn_x_ok(x, x2, B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups) || B > 65535) return RSVLD_EINVAL;
    return gn_scale_shift_impl<InF32>(x, x2, gamma, beta, scale_shift, B, HW, C1, C2, groups, eps, ws, (hipStream_t)stream);
}

extern "C" int rsvld_groupnorm_apply_split(const float* x, const float* x2, void* out, const float* scale_shift,
                                           const float* mod_scale1p, const float* mod_shift, int mod_stride, int B, int HW, int C1,
                                           int C2, int silu, int out_f32, void* stream) {
    if (!out || !scale_shift || !gn_x_ok(x, x2, B, HW, C1, C2) || B > 65535) return RSVLD_EINVAL;
    if (!gn_mod_ok(mod_scale1p, mod_shift, mod_stride, 4)) return RSVLD_EINVAL;
    if (out_f32 < 0 || out_f32 > 3 || (out_f32 == OUT_HQ8 && (C1 + C2) % 32)) return RSVLD_EINVAL;
    with_out_form<OUT_HQ8>(out_f32, [&](auto io) {
        constexpr int OUT = decltype(io)::out_form;
        const int rpb = gn_apply_rows_per_block<decltype(io)>(B, HW, C1, C2);
        hipLaunchKernelGGL(gn_apply_split_kernel<OUT>, dim3((unsigned)cdiv64(HW, rpb), B), dim3(256), 0, (hipStream_t)stream, x, x2,
                           out, scale_shift, mod_scale1p, mod_shift, HW, C1, C2, silu, rpb, mod_stride > 0 ? mod_stride : C1 + C2);
    });
    return rsvld_check_launch();
}

extern "C" int rsvld_layernorm_split(const float* x, void* out, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                                     int out_f32, void* stream) {
    if (!x || !out || rows <= 0 || C <= 0 || C % 8 || C > 4096) return RSVLD_EINVAL;
    if (out_f32 < 0 || out_f32 > 2) return RSVLD_EINVAL;
    with_out_form<OUT_F16>(out_f32, [&](auto io) { launch_layernorm<decltype(io)>(x, out, gamma, beta, rows, C, eps, (hipStream_t)stream); });
    return rsvld_check_launch();
}

extern "C" int rsvld_groupnorm_stats_f32_fast(const float* x, const float* x2, float* mean_var, int B, int HW, int C1, int C2, int groups,
                                              void* ws, void* stream) {
    if (!mean_var || !ws || !gn_align8(ws) || !gn_x_ok(x, x2, B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups) || B > 65535) return RSVLD_EINVAL;
    return gn_stats_impl<InF32>(x, x2, mean_var, B, HW, C1, C2, groups, ws, (hipStream_t)stream);
}

extern "C" int rsvld_groupnorm_scale_shift_from_stats(const float* mean_var, const float* gamma, const float* beta, float* scale_shift,
                                                      int B, int C, int groups, float eps, void* stream) {
    if (!mean_var || !scale_shift || B <= 0 || C <= 0 || groups <= 0 || C % groups) return RSVLD_EINVAL;
    const int total = B * C;
    hipLaunchKernelGGL(gn_ab_from_stats_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean_var, gamma, beta,
                       scale_shift, C, groups, eps, total);
    return rsvld_check_launch();
}
