// gemv.hip -- y[b][n] = sum_k W[n][k] x[b][k] (+ bias[n]) for B = 1 .. RSVLD_DECODE_MAX_ROWS activation rows: the weight-streaming products
// (16-bit weights, or e4m3 bytes with a scale per row and the quantiser that makes them, pack_rows_e4m3_kernel)
// of the caption pass's token loop (reference: models/util.py:17-66 -> llava/model/language_model/llava_llama.py:118-137 -> Llama decode;
// 7 linear layers per decoder layer and the 128 256-row lm_head with M = 1; B > 1: the batched token loop).  One host path -- one validation,
// one launcher -- behind the four entry points, the single-row ones being its B = 1 call; one row runs gemv_kernel / gemv_w8_kernel, two and
// more run gemv_rows_kernel, every row bit-identical to the single-row kernels.
// HBM-bound: every weight byte is read once and used once,
// so there is no LDS tile and no MFMA -- weights go straight to registers in 16-byte pieces (cdna_hip_programming.md section 5,
// "GEMV / M <= 16 decode weights": load straight to VGPRs, deep unroll, late wait), x sits in LDS, accumulation is fp32.
// A wave owns RPW output rows at a time and keeps RPW x 2 sixteen-byte weight loads in flight per lane; the 64 partial sums of a row
// meet in a wave reduction.  Algorithmic bytes = N * K * 2 (+ K * 2 per workgroup for x, from L2).
// Round 5, KS = 4: layers with few output rows (o_proj / down_proj / q|k|v of the 8 B decoder: 4 096 .. 6 144 rows = 256 .. 384 workgroups
// of 16 rows, ONE per CU with 32 KiB of weight loads in flight where ~64 KiB per CU are needed to keep HBM busy) run with the four waves
// of a workgroup SPLITTING K for the same GV_RPW rows: four times the workgroups, partial sums through LDS.
#include "rsvld_common.h"
#include <type_traits>

namespace {

#include "gemv_fused.h"   // GV_WAVES, GV_RPW, gv_stage_x, gv_store, gv_lds_bytes, by_dtype, gv_check: shared with gemv_mma.hip

template <typename T> __device__ __forceinline__ float dot8(const u32x4& w, const u32x4& x, float acc) {
    float wf[8], xf[8];
    unpack8<T>(w, wf);
    unpack8<T>(x, xf);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(wf[e], xf[e], acc);
    return acc;
}

template <typename T, int KS>
__global__ __launch_bounds__(64 * GV_WAVES) void gemv_kernel(const T* __restrict__ W, const T* __restrict__ x, const T* __restrict__ bias,
                                                              T* __restrict__ y, int N, int K, const T* __restrict__ norm_w, float eps,
                                                              const T* __restrict__ residual, int glu) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // x: K elements (+ KS = 4: 4 x GV_RPW partial sums) + 16 floats of reduction scratch
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    gv_stage_x<T>(smem, KS == 4 ? 4 * GV_RPW * (int)sizeof(float) : 0, x, norm_w, eps, K, glu, tid, lane, w);
    auto store = [&](int row, float v) __attribute__((always_inline)) { gv_store<T>(y, bias, residual, row, v); };
    if constexpr (KS == 4) {
        // wave w owns K range [w K/4, (w + 1) K/4) (K % 2048 == 0: whole 512-element steps per wave) of the workgroup's GV_RPW rows
        const int row0 = blockIdx.x * GV_RPW;
        const T* wr[GV_RPW];
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) wr[r] = W + (int64_t)min(row0 + r, N - 1) * K;
        float acc[GV_RPW];
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) acc[r] = 0.f;
        const int kq = K >> 2, kend = (w + 1) * kq;
        int kk = w * kq + lane * 8;
        for (; kk + 512 < kend; kk += 1024) {
            u32x4 wv[2][GV_RPW];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk + u * 512));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const u32x4 xv = *(const u32x4*)(smem + (kk + u * 512) * 2);
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) acc[r] = dot8<T>(wv[u][r], xv, acc[r]);
            }
        }
        for (; kk < kend; kk += 512) {
            const u32x4 xv = *(const u32x4*)(smem + kk * 2);
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) acc[r] = dot8<T>(__builtin_nontemporal_load((const u32x4*)(wr[r] + kk)), xv, acc[r]);
        }
        float* part = (float*)(smem + (size_t)K * 2);
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0) part[w * GV_RPW + r] = v;
        }
        __syncthreads();
        if (tid < GV_RPW && row0 + tid < N) {   // fixed order: wave 0 .. 3
            const float v = ((part[tid] + part[GV_RPW + tid]) + part[2 * GV_RPW + tid]) + part[3 * GV_RPW + tid];
            store(row0 + tid, v);
        }
        return;
    }
    const int row0 = (blockIdx.x * GV_WAVES + w) * GV_RPW;
    if (row0 >= N) return;
    const T* wr[GV_RPW];
#pragma unroll
    for (int r = 0; r < GV_RPW; ++r) wr[r] = W + (int64_t)min(row0 + r, N - 1) * K;   // rows past N re-read the last row, never stored
    float acc[GV_RPW];
#pragma unroll
    for (int r = 0; r < GV_RPW; ++r) acc[r] = 0.f;
    const int steps = K >> 9;                                   // whole 512-element steps (64 lanes x 8 elements)
    int kk = lane * 8;
    for (int s = 0; s + 1 < steps; s += 2, kk += 1024) {        // two steps per iteration: 2 x RPW loads in flight per lane
        u32x4 wv[2][GV_RPW];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk + u * 512));
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const u32x4 xv = *(const u32x4*)(smem + (kk + u * 512) * 2);
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) acc[r] = dot8<T>(wv[u][r], xv, acc[r]);
        }
    }
    for (; kk < K; kk += 512) {                                 // odd step and / or the ragged tail (K % 8 == 0)
        const u32x4 xv = *(const u32x4*)(smem + kk * 2);
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) acc[r] = dot8<T>(__builtin_nontemporal_load((const u32x4*)(wr[r] + kk)), xv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < GV_RPW; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0 && row0 + r < N) store(row0 + r, v);
    }
}

// ---- the same product on OCP e4m3 weights with one power-of-two scale per output row (rsvld_gemv_w8_fused): half the bytes of the loop
// that is bound by nothing else.  y[n] = T(scale[n] * sum_k q[n][k] x'[k] + bias[n]), then the residual; x' is staged exactly as above
// (gv_stage_x) and the result leaves through gv_store, so the three fused forms round where gemv_kernel rounds them.  A 16-byte piece is
// now 16 weights: a wave step covers 1 024 elements of K (64 lanes x 16), two steps are in flight per lane and row as above.  Pieces
// past the end of a wave's K range are skipped per lane (K % 16 == 0: a piece is inside or outside as a whole), which is how both the
// ragged K of the row route and a K quarter that is no whole number of steps (down_proj: 14 336 / 4 = 3.5 steps) are walked.
// (Eight rows per wave instead of GV_RPW = 4 -- twice the loads in flight, half the x' staging per weight byte -- measured 2-8 % SLOWER on
// every decoder shape, A-B-A on one device: the row count stays the 16-bit kernel's.)
template <typename T> __device__ __forceinline__ float dot16_w8(const u32x4& w, const u32x4& x0, const u32x4& x1, float acc) {
    float xf[16];
    unpack8<T>(x0, *(float(*)[8])xf);
    unpack8<T>(x1, *(float(*)[8])(xf + 8));
#pragma unroll
    for (int d = 0; d < 4; ++d) {     // byte j of dword d = element 4 d + j; v_cvt_pk_f32_fp8 takes the low or the high byte pair
        const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
        acc = __builtin_fmaf(lo[0], xf[4 * d], acc);
        acc = __builtin_fmaf(lo[1], xf[4 * d + 1], acc);
        acc = __builtin_fmaf(hi[0], xf[4 * d + 2], acc);
        acc = __builtin_fmaf(hi[1], xf[4 * d + 3], acc);
    }
    return acc;
}

// KS = 1: a wave owns GV_RPW rows over all of K; KS = 4: the four waves of a workgroup split K for the workgroup's GV_RPW rows (K % 64 == 0)
template <typename T, int KS>
__global__ __launch_bounds__(64 * GV_WAVES) void gemv_w8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale, const T* __restrict__ x,
                                                                 const T* __restrict__ bias, T* __restrict__ y, int N, int K,
                                                                 const T* __restrict__ norm_w, float eps, const T* __restrict__ residual, int glu) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // as gemv_kernel: x' (K x 16 bit) (+ KS = 4: partial sums) + reduction scratch
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    gv_stage_x<T>(smem, KS == 4 ? 4 * GV_RPW * (int)sizeof(float) : 0, x, norm_w, eps, K, glu, tid, lane, w);
    const int row0 = KS == 4 ? blockIdx.x * GV_RPW : (blockIdx.x * GV_WAVES + w) * GV_RPW;
    if (KS == 1 && row0 >= N) return;
    const uint8_t* wr[GV_RPW];
#pragma unroll
    for (int r = 0; r < GV_RPW; ++r) wr[r] = W + (int64_t)min(row0 + r, N - 1) * K;   // rows past N re-read the last row, never stored
    float acc[GV_RPW];
#pragma unroll
    for (int r = 0; r < GV_RPW; ++r) acc[r] = 0.f;
    const int kq = K >> 2, kend = KS == 4 ? (w + 1) * kq : K;
    int kb = KS == 4 ? w * kq : 0;
    for (; kb + 2048 <= kend; kb += 2048) {                     // two whole steps per iteration: 2 x RPW loads in flight per lane
        const int kk = kb + lane * 16;
        u32x4 wv[2][GV_RPW];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk + u * 1024));
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const u32x4 x0 = *(const u32x4*)(smem + (kk + u * 1024) * 2), x1 = *(const u32x4*)(smem + (kk + u * 1024) * 2 + 16);
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) acc[r] = dot16_w8<T>(wv[u][r], x0, x1, acc[r]);
        }
    }
    for (; kb < kend; kb += 1024) {                             // the odd step and / or the ragged tail, piece by piece
        const int kk = kb + lane * 16;
        if (kk < kend) {
            u32x4 wv[GV_RPW];
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) wv[r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk));
            const u32x4 x0 = *(const u32x4*)(smem + kk * 2), x1 = *(const u32x4*)(smem + kk * 2 + 16);
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) acc[r] = dot16_w8<T>(wv[r], x0, x1, acc[r]);
        }
    }
    if constexpr (KS == 4) {
        float* part = (float*)(smem + (size_t)K * 2);
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0) part[w * GV_RPW + r] = v;
        }
        __syncthreads();
        if (tid < GV_RPW && row0 + tid < N) {   // fixed order: wave 0 .. 3
            const float v = ((part[tid] + part[GV_RPW + tid]) + part[2 * GV_RPW + tid]) + part[3 * GV_RPW + tid];
            gv_store<T>(y, bias, residual, row0 + tid, v * scale[row0 + tid]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0 && row0 + r < N) gv_store<T>(y, bias, residual, row0 + r, v * scale[row0 + r]);
        }
    }
}

// ---- the quantiser of those weights (rsvld_pack_rows_e4m3): a wave owns a row.  Pass 1: amax over the row's FINITE elements (wave
// reduction); e = the smallest integer with amax 2^-e <= 448 = 0.875 x 2^9, read off amax's exponent and mantissa bits (amax = m 2^x,
// m in [0.5, 1): e = x - 9 if m <= 0.875, else x - 8; no logarithm), 0 for an all-zero row, clamped to [-126, 127].  Pass 2 (the row
// comes back from L2): q = e4m3_rne(w 2^-e) -- an exact scaling, nothing saturates -- and byte 0x7F (e4m3 NaN) for a non-finite weight.
template <typename T>
__global__ __launch_bounds__(64 * GV_WAVES) void pack_rows_e4m3_kernel(const T* __restrict__ W, uint8_t* __restrict__ q, float* __restrict__ scale,
                                                                        int N, int K) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * GV_WAVES + (threadIdx.x >> 6);
    if (row >= N) return;
    const T* wr = W + (int64_t)row * K;
    uint8_t* qr = q + (int64_t)row * K;
    float amax = 0.f;
    for (int kk = lane * 16; kk < K; kk += 1024) {
        float f[16];
        unpack8<T>(*(const u32x4*)(wr + kk), *(float(*)[8])f);
        unpack8<T>(*(const u32x4*)(wr + kk + 8), *(float(*)[8])(f + 8));
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float a = fabsf(f[e]);
            amax = a < INFINITY ? fmaxf(amax, a) : amax;        // (NaN and Inf compare false)
        }
    }
    amax = wave_max(amax);
    int e = 0;
    if (amax > 0.f) {
        const uint32_t b = __builtin_bit_cast(uint32_t, amax);
        int E = (int)(b >> 23);
        uint32_t man = b & 0x7FFFFFu;
        if (E == 0) {                                           // an fp32 subnormal (a bf16 one): normalise
            const int sh = __builtin_clz(man) - 8;
            man = (man << sh) & 0x7FFFFFu;
            E = 1 - sh;
        }
        // amax = (1 + man 2^-23) 2^(E - 127) = m 2^x with x = E - 126; m <= 0.875 <=> man <= 0.75 x 2^23
        e = (E - 126) - (man <= 0x600000u ? 9 : 8);
        e = min(max(e, -126), 127);
    }
    const float inv = e < 127 ? __builtin_bit_cast(float, (uint32_t)(127 - e) << 23) : __builtin_bit_cast(float, 0x00400000u);   // 2^-e
    if (lane == 0) scale[row] = __builtin_bit_cast(float, (uint32_t)(127 + e) << 23);
    for (int kk = lane * 16; kk < K; kk += 1024) {
        float f[16];
        unpack8<T>(*(const u32x4*)(wr + kk), *(float(*)[8])f);
        unpack8<T>(*(const u32x4*)(wr + kk + 8), *(float(*)[8])(f + 8));
        u32x4 out;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t v = cvt4_e4m3(f[4 * d] * inv, f[4 * d + 1] * inv, f[4 * d + 2] * inv, f[4 * d + 3] * inv);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(fabsf(f[4 * d + j]) < INFINITY)) v = (v & ~(0xFFu << (8 * j))) | (0x7Fu << (8 * j));
            out[d] = v;
        }
        *(u32x4*)(qr + kk) = out;
    }
}

// ---- the same products for NB activation rows at once (rsvld_gemv_rows_fused, rsvld_gemv_w8_rows_fused): the batched token loop streams a
// weight piece ONCE into registers and uses it for every row.  Per activation row the arithmetic is gemv_kernel's / gemv_w8_kernel's, operation
// for operation: the row is staged by gv_stage_x (its own K elements of LDS), lane l of a wave accumulates the same k in the same ascending
// order with the same fmaf chain (dot8 / dot16_w8) into an accumulator of its own, the 64 partial sums meet in the same wave_sum, the K-split
// route adds its four partials in the same fixed order, and the result leaves through gv_store -- so row b of the result is bit for bit what
// the single-row kernel gives for x[b], whatever NB is and whatever the other rows hold (a NaN row stays in its own accumulators).  What may
// differ is only WHICH workgroup computes an output row: a workgroup keeps its staged rows and walks output-row blocks blk, blk + gridDim.x, ..
// (the staging of NB rows is paid once per workgroup, not once per 16 output rows).  The conversions of a weight piece to fp32 are written
// inside dot8 / dot16_w8 per row; unrolled, the compiler keeps one copy per piece.
// LDS: [NB][K] x' | KS = 4: [NB][4][GV_RPW] partial sums | 16 floats of reduction scratch.
// (at least two waves per SIMD: left alone, the compiler spends 512 registers per lane on the eight-row form -- one workgroup per CU, nothing
// to hide a weight load behind)
constexpr int GVR_MIN_WAVES = 2;
// rows up to which two weight steps are in flight per lane, as in the single-row kernels; with more rows the converted pieces of two steps
// and the accumulators no longer fit the registers of two waves per SIMD (spills), and the loop is bound by its arithmetic anyway
constexpr int GVR_TWO_STEP_ROWS = 2;
template <typename T, int KS, int NB, bool W8>
__global__ __launch_bounds__(64 * GV_WAVES, GVR_MIN_WAVES) void gemv_rows_kernel(const void* __restrict__ Wv, const float* __restrict__ scale, const T* __restrict__ x,
                                                                   const T* __restrict__ bias, T* __restrict__ y, int N, int K,
                                                                   const T* __restrict__ norm_w, float eps, const T* __restrict__ residual, int glu,
                                                                   int nblocks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using W = std::conditional_t<W8, uint8_t, T>;
    constexpr int PIECE = W8 ? 16 : 8, STEP = 64 * PIECE;      // elements of K per 16-byte piece / per wave step
    const W* Wm = (const W*)Wv;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t xrow = (size_t)K * 2;                          // bytes of one staged row
    const int part_bytes = KS == 4 ? NB * 4 * GV_RPW * (int)sizeof(float) : 0;
#pragma unroll
    for (int b = 0; b < NB; ++b)                                // (red_off: every row's reduction scratch is the one behind the partial sums)
        gv_stage_x<T>(smem + b * xrow, (NB - 1 - b) * (int)xrow + part_bytes, x + (size_t)b * (glu ? 2 * K : K), norm_w, eps, K, glu, tid, lane, w);
    float* part = (float*)(smem + NB * xrow);
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int row0 = KS == 4 ? blk * GV_RPW : (blk * GV_WAVES + w) * GV_RPW;
        if (KS == 1 && row0 >= N) continue;
        const W* wr[GV_RPW];
#pragma unroll
        for (int r = 0; r < GV_RPW; ++r) wr[r] = Wm + (int64_t)min(row0 + r, N - 1) * K;   // rows past N re-read the last row, never stored
        float acc[NB][GV_RPW];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < GV_RPW; ++r) acc[b][r] = 0.f;
        // one piece of each of the GV_RPW weight rows against every staged row
        auto fma_rows = [&](const u32x4 (&wv)[GV_RPW], int kk) __attribute__((always_inline)) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const char* xs = smem + b * xrow + (size_t)kk * 2;
                if constexpr (W8) {
                    const u32x4 x0 = *(const u32x4*)xs, x1 = *(const u32x4*)(xs + 16);
#pragma unroll
                    for (int r = 0; r < GV_RPW; ++r) acc[b][r] = dot16_w8<T>(wv[r], x0, x1, acc[b][r]);
                } else {
                    const u32x4 xv = *(const u32x4*)xs;
#pragma unroll
                    for (int r = 0; r < GV_RPW; ++r) acc[b][r] = dot8<T>(wv[r], xv, acc[b][r]);
                }
            }
        };
        // the K range of this wave and its lane's first piece: as gemv_kernel / gemv_w8_kernel
        const int kq = K >> 2, kend = KS == 4 ? (w + 1) * kq : K;
        int kk = (KS == 4 ? w * kq : 0) + lane * PIECE;
        const int kbeg = kk - lane * PIECE;
        // two whole steps per iteration (2 x GV_RPW loads in flight per lane), then step by step with pieces past the range skipped per
        // lane: the same ascending k sequence per lane as the single-row loops, whose own two-step / tail split is not part of the result
        int kb = kbeg;
        if constexpr (NB <= GVR_TWO_STEP_ROWS) for (; kb + 2 * STEP <= kend; kb += 2 * STEP, kk += 2 * STEP) {
            u32x4 wv[2][GV_RPW];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk + u * STEP));
#pragma unroll
            for (int u = 0; u < 2; ++u) fma_rows(wv[u], kk + u * STEP);
        }
        for (; kb < kend; kb += STEP, kk += STEP) {
            if (kk < kend) {
                u32x4 wv[GV_RPW];
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) wv[r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + kk));
                fma_rows(wv, kk);
            }
        }
        if constexpr (KS == 4) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) {
                    const float v = wave_sum(acc[b][r]);
                    if (lane == 0) part[(b * 4 + w) * GV_RPW + r] = v;
                }
            __syncthreads();
            if (tid < NB * GV_RPW && row0 + (tid % GV_RPW) < N) {   // fixed order: wave 0 .. 3
                const int b = tid / GV_RPW, r = tid % GV_RPW;
                const float* pb = part + b * 4 * GV_RPW;
                float v = ((pb[r] + pb[GV_RPW + r]) + pb[2 * GV_RPW + r]) + pb[3 * GV_RPW + r];
                if constexpr (W8) v = v * scale[row0 + r];
                gv_store<T>(y + (size_t)b * N, bias, residual != nullptr ? residual + (size_t)b * N : nullptr, row0 + r, v);
            }
            __syncthreads();                                     // the partial sums are rewritten by the next block of rows
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < GV_RPW; ++r) {
                    float v = wave_sum(acc[b][r]);
                    if (lane == 0 && row0 + r < N) {
                        if constexpr (W8) v = v * scale[row0 + r];
                        gv_store<T>(y + (size_t)b * N, bias, residual != nullptr ? residual + (size_t)b * N : nullptr, row0 + r, v);
                    }
                }
        }
    }
}

// ---- host side of the products: one validation (gv_check), one launcher (gvr_launch) for the four entry points
// The row / K-split route of an (N, K) product, stated once.  The number of activation rows must not enter it: a row's summation order is
// the route's.  Few output rows (fewer than ~4 row-split workgroups per CU of a 256-CU chip): the four waves of a workgroup split K --
// 16-bit weights where a quarter of K is whole wave steps, e4m3 for every K whose quarter is whole 16-element pieces (K % 64 == 0) and at
// least two wave steps long in all (K >= 2 048).
bool gemv_ksplit(int N, int K) { return K % 2048 == 0 && (N + GV_WAVES * GV_RPW - 1) / (GV_WAVES * GV_RPW) < 1024; }
bool gemv_w8_ksplit(int N, int K) { return K % 64 == 0 && K >= 2048 && (N + GV_WAVES * GV_RPW - 1) / (GV_WAVES * GV_RPW) < 1024; }

// a group of NB >= 2 rows: gemv_rows_kernel on a persistent grid of what the chip holds at once
template <typename T, int KS, int NB, bool W8>
int gvr_go(const void* w, const float* scale, const void* x, const void* bias, const void* norm_w, float eps, const void* residual, int glu,
           void* y, int N, int K, hipStream_t s) {
    constexpr auto KERN = gemv_rows_kernel<T, KS, NB, W8>;
    const size_t smem = gv_lds_bytes(K, NB, KS == 4);
    if (smem > 65536 && rsvld_smem_once<KERN>(GVR_LDS) != hipSuccess) return RSVLD_ELAUNCH;
    const int nblocks = KS == 4 ? (N + GV_RPW - 1) / GV_RPW : (N + GV_WAVES * GV_RPW - 1) / (GV_WAVES * GV_RPW);
    const int per_cu = (int)(GVR_LDS / smem) < 8 ? (int)(GVR_LDS / smem) : 8;     // workgroups of 4 waves a CU holds
    const int grid = nblocks < GVR_CUS * per_cu ? nblocks : GVR_CUS * per_cu;
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(64 * GV_WAVES), smem, s, w, scale, (const T*)x, (const T*)bias, (T*)y, N, K, (const T*)norm_w, eps,
                       (const T*)residual, glu, nblocks);
    return RSVLD_OK;
}
// one row: the single-row kernels, a workgroup per block of output rows.  (gemv_rows_kernel<.., NB = 1, ..> gives the same bits and is not
// instantiated: merged into one template with these two, its NB = 1 form timed 0.4-0.5 us above them on down_proj e4m3 and gate|up native,
// same weight memory, profiles/gemv_merge_ab.txt -- so one row keeps the kernels it had, and B = 1 of the rows entry points gets them too.)
template <typename T, int KS, bool W8>
int gv_one(const void* w, const float* scale, const void* x, const void* bias, const void* norm_w, float eps, const void* residual, int glu,
           void* y, int N, int K, hipStream_t s) {
    const dim3 grid((unsigned)(KS == 4 ? (N + GV_RPW - 1) / GV_RPW : (N + GV_WAVES * GV_RPW - 1) / (GV_WAVES * GV_RPW))), block(64 * GV_WAVES);
    const size_t smem = gv_lds_bytes(K, 1, KS == 4);
    if constexpr (W8) hipLaunchKernelGGL((gemv_w8_kernel<T, KS>), grid, block, smem, s, (const uint8_t*)w, scale, (const T*)x, (const T*)bias, (T*)y, N, K,
                                         (const T*)norm_w, eps, (const T*)residual, glu);
    else hipLaunchKernelGGL((gemv_kernel<T, KS>), grid, block, smem, s, (const T*)w, (const T*)x, (const T*)bias, (T*)y, N, K, (const T*)norm_w, eps,
                            (const T*)residual, glu);
    return RSVLD_OK;
}
// One instantiation per row count from two on: 2 types x 2 routes x 7 row counts x 2 weight kinds = 56 kernels, each unrolled over its rows.  Cost,
// measured on this file: it compiles in ~30 s instead of ~4 s and its object grows from 0.12 to 1.4 MB.  The alternative -- only 2 / 4 / 8
// rows, a group rounded up and the surplus rows masked at the store -- would spend the surplus rows' arithmetic, which is what binds from
// four rows on (3 rows at the price of 4, 5 at the price of 8): not taken.  Every count is reachable: B itself, and the groups of gvr_launch.
template <typename T, int KS, bool W8, typename... A> int gvr_nb(int nb, A... a) {
    switch (nb) {
        case 1: return gv_one<T, KS, W8>(a...);
        case 2: return gvr_go<T, KS, 2, W8>(a...);
        case 3: return gvr_go<T, KS, 3, W8>(a...);
        case 4: return gvr_go<T, KS, 4, W8>(a...);
        case 5: return gvr_go<T, KS, 5, W8>(a...);
        case 6: return gvr_go<T, KS, 6, W8>(a...);
        case 7: return gvr_go<T, KS, 7, W8>(a...);
        case 8: return gvr_go<T, KS, 8, W8>(a...);
    }
    return RSVLD_EINVAL;
}

// The product for B rows (B = 1: the single-row entry points), checked, in groups of equal size whose staged rows fit the LDS (K <= 10 200:
// one group of eight; down_proj's K = 14 336: 2 x 4; the largest K gv_check takes: 4 x 2) -- a group is one launch, and one pass over the weights
template <bool W8>
int gvr_launch(const void* w, const float* scale, const void* x, const void* bias, const void* norm_w, float eps, const void* residual, int glu,
               void* y, int N, int K, int B, int dtype, void* stream) {
    if (const int rc = gv_check<W8>(w, scale, x, norm_w, glu, y, N, K, B, dtype); rc != RSVLD_OK) return rc;
    glu = glu ? 1 : 0;
    const bool ksplit = W8 ? gemv_w8_ksplit(N, K) : gemv_ksplit(N, K);
    const size_t scratch = gv_lds_bytes(K, 0, true), per_row = gv_lds_bytes(K, 1, true) - scratch;
    const int fit = (int)((GVR_LDS - scratch) / per_row);                      // >= 2: a single row is <= 64 KiB
    const int gmax = fit < RSVLD_DECODE_MAX_ROWS ? fit : RSVLD_DECODE_MAX_ROWS;
    const int ngroups = (B + gmax - 1) / gmax, g = (B + ngroups - 1) / ngroups;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += g) {
        const int nb = B - b0 < g ? B - b0 : g;
        const char* xg = (const char*)x + (size_t)b0 * (glu ? 2 : 1) * K * 2;
        const char* rg = residual ? (const char*)residual + (size_t)b0 * N * 2 : nullptr;
        char* yg = (char*)y + (size_t)b0 * N * 2;
        const int rc = by_dtype(dtype, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            return ksplit ? gvr_nb<T, 4, W8>(nb, w, scale, xg, bias, norm_w, eps, rg, glu, yg, N, K, s)
                          : gvr_nb<T, 1, W8>(nb, w, scale, xg, bias, norm_w, eps, rg, glu, yg, N, K, s);
        });
        if (rc != RSVLD_OK) return rc;
    }
    return rsvld_check_launch();
}

}  // namespace

extern "C" int rsvld_pack_rows_e4m3(const void* w, void* q, float* scale, int N, int K, int dtype, void* stream) {
    if (!w || !q || !scale || N <= 0 || K <= 0) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (K % 16 != 0) return RSVLD_EUNSUPPORTED;   // 16-byte pieces of q
    if ((((uintptr_t)w | (uintptr_t)q) & 15) || ((uintptr_t)scale & 3)) return RSVLD_EINVAL;
    const dim3 grid((unsigned)((N + GV_WAVES - 1) / GV_WAVES));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSVLD_F16) hipLaunchKernelGGL((pack_rows_e4m3_kernel<f16>), grid, dim3(64 * GV_WAVES), 0, s, (const f16*)w, (uint8_t*)q, scale, N, K);
    else hipLaunchKernelGGL((pack_rows_e4m3_kernel<bf16>), grid, dim3(64 * GV_WAVES), 0, s, (const bf16*)w, (uint8_t*)q, scale, N, K);
    return rsvld_check_launch();
}

// ---- the products' entry points: the single-row ones are the B = 1 call
extern "C" int rsvld_gemv_rows_fused(const void* w, const void* x, const void* bias, const void* norm_w, float norm_eps, const void* residual,
                                     int glu, void* y, int N, int K, int B, int dtype, void* stream) {
    return gvr_launch<false>(w, nullptr, x, bias, norm_w, norm_eps, residual, glu, y, N, K, B, dtype, stream);
}

extern "C" int rsvld_gemv_w8_rows_fused(const void* q, const float* scale, const void* x, const void* bias, const void* norm_w, float norm_eps,
                                        const void* residual, int glu, void* y, int N, int K, int B, int dtype, void* stream) {
    return gvr_launch<true>(q, scale, x, bias, norm_w, norm_eps, residual, glu, y, N, K, B, dtype, stream);
}

extern "C" int rsvld_gemv(const void* w, const void* x, const void* bias, void* y, int N, int K, int dtype, void* stream) {
    return rsvld_gemv_rows_fused(w, x, bias, nullptr, 0.f, nullptr, 0, y, N, K, 1, dtype, stream);
}

extern "C" int rsvld_gemv_fused(const void* w, const void* x, const void* bias, const void* norm_w, float norm_eps, const void* residual, int glu,
                                void* y, int N, int K, int dtype, void* stream) {
    return rsvld_gemv_rows_fused(w, x, bias, norm_w, norm_eps, residual, glu, y, N, K, 1, dtype, stream);
}

extern "C" int rsvld_gemv_w8_fused(const void* q, const float* scale, const void* x, const void* bias, const void* norm_w, float norm_eps,
                                   const void* residual, int glu, void* y, int N, int K, int dtype, void* stream) {
    return rsvld_gemv_w8_rows_fused(q, scale, x, bias, norm_w, norm_eps, residual, glu, y, N, K, 1, dtype, stream);
}
