// gemm_w8.hip -- out[m][n] = T(scale[n] * sum_k x[m][k] e4m3(q[n][k]) + bias[n]) for M rows of 16-bit activations against the e4m3 packs
// of rsvld_pack_rows_e4m3: the projections of the caption pass's PREFILL on the weights its token loop streams (the _lin calls of
// llava_next.FastDecoder.forward at T > 1: q|k|v, o_proj, gate|up, down_proj), so that a caption is ONE model from the first prompt
// token to the last generated one and the 16-bit decoder weights need not stay resident.
//
// A tile GEMM on the 32x32x16 16-bit MFMAs, fp32 accumulation.  A workgroup (4 waves, 2 x 2) owns GW_BM x GW_BN = 128 x 128 outputs, a
// wave 64 x 64 of them (2 x 2 accumulators), and walks K in ascending steps of GW_BK = 64.  Both operands are staged THROUGH REGISTERS
// into a double-buffered LDS image of 16-bit elements:
//   * x: 16-byte pieces of 8 elements, copied as they are;
//   * q: 16-byte pieces of 16 e4m3 bytes, converted to T ON THE WAY INTO LDS (v_cvt_pk_f32_fp8, then fp32 -> T: every e4m3 value is
//     exact in fp16 and in bf16, so the operand is q UNSCALED -- q 2^e is not always representable in fp16, the scale is applied to the
//     fp32 sum in the epilogue).  A weight byte is therefore converted once per workgroup and used by all 128 rows of the tile; converting
//     behind LDS would halve the LDS bytes of the weights but repeat the conversion in both waves that share a weight fragment, in a
//     loop whose VALU slots are what the MFMAs leave over.
// The loads of step t + 1 are issued before the MFMAs of step t and written to the other buffer after them: one barrier per step.
// LDS rows are 128 bytes (64 elements); 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 7), so the 16 rows a quarter of a
// ds_read_b128 wavefront reads (same c) fall into the 16 distinct 16-byte positions of the 256-byte bank period.
// x is the MFMA's A operand (D row = m, on the accumulator registers), q its B operand (D column = n, on the lane): a lane's 16 results
// of an accumulator share one n -- one scale, one bias -- and a store instruction writes 32 consecutive n of a row.
//
// ROW INVARIANCE (the contract in include/rsvld_hip.h): the tile, the K order and the MFMA shape are constants of this file -- nothing
// is chosen from M, there is no split over K -- and an MFMA output element is a function of its own A row and B column.  Rows past M,
// columns past N and K pieces past K (K % 16 == 0: a piece is inside or outside as a whole) are ZEROS in LDS, never loaded; their
// results are not stored.  A NaN in another row of x stays in that row's accumulators.
#include "rsvld_common.h"
#include "rsvld_plan.h"

namespace {

using rsvld_plan::GW_BM;
using rsvld_plan::GW_BN;
using rsvld_plan::GW_BK;
constexpr int GW_ROWB = GW_BK * 2;                    // bytes of an LDS row
constexpr int GW_XS = GW_BM * GW_ROWB, GW_WS = GW_BN * GW_ROWB;
constexpr int GW_XP = GW_BM * GW_BK / 8 / 256;        // 16-byte pieces of x per thread and step (4)
constexpr int GW_WP = GW_BN * GW_BK / 16 / 256;       // 16-byte pieces of q per thread and step (2)
static_assert(GW_BM == 128 && GW_BN == 128 && GW_BK == 64, "the wave layout and the staging maps below are written for 128 x 128 x 64");

__device__ __forceinline__ int gw_off(int row, int chunk) { return row * GW_ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

// 8 e4m3 bytes (two dwords; byte j of dword d = element 4 d + j) -> 8 x T, exact
template <typename T> __device__ __forceinline__ u32x4 gw_cvt8(uint32_t d0, uint32_t d1) {
    typename Mfma<T>::v8 v;
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, true);
    const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, true);
    v[0] = (T)a[0]; v[1] = (T)a[1]; v[2] = (T)b[0]; v[3] = (T)b[1];
    v[4] = (T)c[0]; v[5] = (T)c[1]; v[6] = (T)d[0]; v[7] = (T)d[1];
    return __builtin_bit_cast(u32x4, v);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void gemm_w8_kernel(const T* __restrict__ x, const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                         const T* __restrict__ bias, T* __restrict__ out, int M, int N, int K) {
    typedef typename Mfma<T>::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[2 * (GW_XS + GW_WS)];   // [buffer][x tile | converted q tile]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = w & 1, wn = w >> 1;                   // the wave's 64 x 64 quadrant
    const int m0 = blockIdx.x * GW_BM, n0 = blockIdx.y * GW_BN;

    // ---- staging maps.  x: thread (row tid >> 3 + 32 i, chunk tid & 7); q: thread (row tid >> 2 + 64 i, piece tid & 3 = chunks 2 p, 2 p + 1)
    const int xc = tid & 7, wp = tid & 3;
    const T* xsrc[GW_XP];
    const uint8_t* wsrc[GW_WP];
    int xdst[GW_XP], wdst[GW_WP][2];
#pragma unroll
    for (int i = 0; i < GW_XP; ++i) {
        const int r = (tid >> 3) + 32 * i;
        xsrc[i] = m0 + r < M ? x + (int64_t)(m0 + r) * K + xc * 8 : nullptr;
        xdst[i] = gw_off(r, xc);
    }
#pragma unroll
    for (int i = 0; i < GW_WP; ++i) {
        const int r = (tid >> 2) + 64 * i;
        wsrc[i] = n0 + r < N ? q + (int64_t)(n0 + r) * K + wp * 16 : nullptr;
        wdst[i][0] = GW_XS + gw_off(r, 2 * wp);
        wdst[i][1] = GW_XS + gw_off(r, 2 * wp + 1);
    }
    u32x4 xv[GW_XP], wv[GW_WP];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    auto load = [&](int t) __attribute__((always_inline)) {
        const int k0 = t * GW_BK;
#pragma unroll
        for (int i = 0; i < GW_XP; ++i) xv[i] = (xsrc[i] != nullptr && k0 + xc * 8 < K) ? *(const u32x4*)(xsrc[i] + k0) : zero;
#pragma unroll
        for (int i = 0; i < GW_WP; ++i) wv[i] = (wsrc[i] != nullptr && k0 + wp * 16 < K) ? *(const u32x4*)(wsrc[i] + k0) : zero;
    };
    auto stage = [&](int buf) __attribute__((always_inline)) {
        char* s = smem + buf * (GW_XS + GW_WS);
#pragma unroll
        for (int i = 0; i < GW_XP; ++i) *(u32x4*)(s + xdst[i]) = xv[i];
#pragma unroll
        for (int i = 0; i < GW_WP; ++i) {
            *(u32x4*)(s + wdst[i][0]) = gw_cvt8<T>(wv[i][0], wv[i][1]);
            *(u32x4*)(s + wdst[i][1]) = gw_cvt8<T>(wv[i][2], wv[i][3]);
        }
    };

    // ---- fragment read offsets: lane (row l31, k = 8 lh + j) of k-step ks reads chunk 2 ks + lh of its row
    int aoff[2][4], boff[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            aoff[i][ks] = gw_off(wm * 64 + i * 32 + l31, 2 * ks + lh);
            boff[i][ks] = GW_XS + gw_off(wn * 64 + i * 32 + l31, 2 * ks + lh);
        }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (K + GW_BK - 1) / GW_BK;
    load(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const bool more = t + 1 < nk;
        if (more) load(t + 1);                           // in flight under this step's MFMAs
        const char* s = smem + (t & 1) * (GW_XS + GW_WS);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            v8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *(const v8*)(s + aoff[i][ks]);
                b[i] = *(const v8*)(s + boff[i][ks]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::mma(a[i], b[j], acc[i][j]);
        }
        if (more) stage((t + 1) & 1);                    // the buffer step t - 1 was read from: everyone passed the last barrier since
        __syncthreads();
    }

    // ---- epilogue: scale and bias in fp32, ONE rounding to T.  acc[i][j]: rows m0 + 64 wm + 32 i + (r & 3) + 8 (r >> 2) + 4 lh, column n0 + 64 wn + 32 j + l31
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + l31;
        if (n >= N) continue;
        const float sc = scale[n], bs = bias != nullptr ? (float)bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < M) out[(int64_t)m * N + n] = (T)(acc[i][j][r] * sc + bs);
            }
    }
}

}  // namespace

extern "C" int rsvld_plan_gemm_w8(int M, int N, int K, int dtype, rsvld_gemm_w8_plan* plan) {
    if (plan == nullptr) return RSVLD_EINVAL;
    return rsvld_plan::plan_gemm_w8(M, N, K, dtype, plan);
}

extern "C" int rsvld_gemm_w8(const void* x, const uint8_t* q, const float* scale, const void* bias, void* out, int M, int N, int K, int dtype,
                             void* stream) {
    if (!x || !q || !scale || !out) return RSVLD_EINVAL;
    rsvld_gemm_w8_plan pl;
    if (const int rc = rsvld_plan::plan_gemm_w8(M, N, K, dtype, &pl); rc != RSVLD_OK) return rc;
    // 16-byte pieces of x and q (K % 16 == 0 keeps every row of both aligned); scale is read as fp32, bias and out element by element
    if ((((uintptr_t)x | (uintptr_t)q) & 15) || ((uintptr_t)scale & 3) || (((uintptr_t)bias | (uintptr_t)out) & 1)) return RSVLD_EINVAL;
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(64 * pl.waves);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSVLD_F16)
        hipLaunchKernelGGL(gemm_w8_kernel<f16>, grid, block, 0, s, (const f16*)x, q, scale, (const f16*)bias, (f16*)out, M, N, K);
    else
        hipLaunchKernelGGL(gemm_w8_kernel<bf16>, grid, block, 0, s, (const bf16*)x, q, scale, (const bf16*)bias, (bf16*)out, M, N, K);
    return rsvld_check_launch();
}
