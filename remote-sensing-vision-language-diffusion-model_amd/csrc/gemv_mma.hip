// gemv_mma.hip -- the decode products of gemv.hip, y[b][n] = T(scale[n] sum_k W[n][k] x'[b][k] + bias[n]) (+ residual) for B = 1 ..
// RSVLD_DECODE_MAX_ROWS activation rows, on MFMAs (rsvld_gemv_mma_rows_fused, rsvld_gemv_w8_mma_rows_fused; opt-in: FastDecoder(decode="mfma")).
// gemv_rows_kernel runs one fmaf chain per activation row and weight element on the VALU, which binds from four rows on; here one
// v_mfma_f32_16x16x32 takes 16 weight rows x 32 k (the A operand) against up to 16 activation rows (the columns of the B operand), so the
// arithmetic of eight rows costs what one row costs and the step is bound by weight bytes again.
// CONTRACT (tests/test_gpu_gemv_mma.py): MFMA columns are independent, columns c >= B are zero REGISTERS (never read from LDS, never
// stored), and the route (rsvld_plan::plan_gemv_mma) is a function of (N, K, weight kind) -- so row b of the result is bit for bit the
// same for every B and whatever the other rows hold.  x' is staged by gv_stage_x and the result leaves through gv_store (gemv_fused.h):
// against the VALU kernels only the order of the fp32 sum differs.
//
// How a weight byte reaches the A operand.  The MFMA layout puts 16 different weight rows on adjacent lanes; a global load in that layout
// would touch 16 cache lines per quarter-wave with 16 bytes each.  So the load stays the VALU kernels': 16-byte pieces, lanes consecutive
// in k along a weight row (32 lanes = 512 contiguous bytes of a row, two rows per wave instruction), nontemporal -- and the transposition
// goes through a slab of LDS that belongs to ONE wave: GM_ROWS rows x GM_STEP_BYTES, written as loaded (ds_write_b128) and read back in
// fragment layout (ds_read_b128: lane l takes row l & 15, piece 4 m + (l >> 4) of k-chunk m).  Piece p of row r sits at piece p ^ r: the
// 16 lanes of a ds_read_b128 lane group (8 rows of one k group, 8 of another) then cover the 16 sixteen-byte slots of the 256-byte bank
// row once, and the 8 lanes of a ds_write_b128 group still write 128 contiguous bytes.  A wave's LDS operations execute in order, so
// the K loop has no workgroup barrier: only the staging and the K-split combine have.  Per CU and clock the slab moves the ~11 bytes of
// the HBM stream in and out, against ~79 B/clk of ds_write_b128 and 256 B/clk of reads.
// A wave keeps TWO steps of loads in flight (the next step is requested before the current one is written to the slab): 16 KiB per wave,
// 64 KiB per workgroup -- what HBM needs per CU on this chip (gemv.hip) even where the staged rows leave room for one workgroup only.
// e4m3 bytes pass the slab as bytes (a step is 512 k instead of 256) and are converted after the fragment read (v_cvt_pk_f32_fp8, then to
// T: exact, UNSCALED); scale[n] meets the fp32 sum in the epilogue, as in gemv_w8_kernel and gemm_w8.  A 16-byte fragment read holds a lane's
// operands of two MFMAs: k = 64 c + 16 g + (0..7 | 8..15) for lane group g -- the B operand is read in the same order.
// The K tail: a piece past the end of a wave's K range is zeros in the registers of BOTH operands (a piece is in or out as a whole:
// K % 8 / K % 16), weight rows past N re-read row N - 1 and are never stored.
#include "rsvld_common.h"
#include "rsvld_plan.h"
#include <type_traits>

namespace {

#include "gemv_fused.h"

using rsvld_plan::GM_ROWS;
using rsvld_plan::GM_WAVES;
using rsvld_plan::GM_STEP_BYTES;
using rsvld_plan::GM_SLAB;
static_assert(GM_WAVES == GV_WAVES, "gv_stage_x stages with GV_WAVES waves");
constexpr int GM_LOADS = GM_SLAB / (64 * 16);     // 16-byte loads per lane and step (8)
constexpr int GM_MIN_WAVES = 2;                   // waves per SIMD the register budget leaves room for

template <typename T> __device__ __forceinline__ f32x4 gm_mma(typename Mfma<T>::v8 a, typename Mfma<T>::v8 b, f32x4 c) {
    if constexpr (std::is_same_v<T, f16>) return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// 8 e4m3 bytes (two dwords; byte j of dword d = element 4 d + j) -> 8 x T, exact
template <typename T> __device__ __forceinline__ typename Mfma<T>::v8 gm_cvt8(uint32_t d0, uint32_t d1) {
    typename Mfma<T>::v8 v;
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, true);
    const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, true);
    v[0] = (T)a[0]; v[1] = (T)a[1]; v[2] = (T)b[0]; v[3] = (T)b[1];
    v[4] = (T)c[0]; v[5] = (T)c[1]; v[6] = (T)d[0]; v[7] = (T)d[1];
    return v;
}

// LDS: [nb staged rows, xstride apart] | 16 floats of reduction scratch | KSPLIT: GM_WAVES x 16 x 16 partial sums | GM_WAVES slabs
template <typename T, bool KSPLIT, bool W8>
__global__ __launch_bounds__(64 * GM_WAVES, GM_MIN_WAVES) void gemv_mma_kernel(const void* __restrict__ Wv, const float* __restrict__ scale,
                                                                                 const T* __restrict__ x, const T* __restrict__ bias,
                                                                                 T* __restrict__ y, int N, int K, const T* __restrict__ norm_w,
                                                                                 float eps, const T* __restrict__ residual, int glu, int nb,
                                                                                 int nblocks, int xstride, int steps_per_way) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using V8 = typename Mfma<T>::v8;
    constexpr int EB = W8 ? 1 : 2;                              // bytes per weight element
    constexpr int PIECE = 16 / EB, KSTEP = GM_STEP_BYTES / EB;  // elements of K per 16-byte piece / per step
    const char* Wm = (const char*)Wv;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int b = 0; b < nb; ++b)                                // (red_off: every row's reduction scratch is the one behind the last row)
        gv_stage_x<T>(smem + (size_t)b * xstride, (nb - b) * xstride - K * 2, x + (size_t)b * (glu ? 2 * K : K), norm_w, eps, K, glu, tid, lane, w);
    float* part = (float*)(smem + (size_t)nb * xstride + rsvld_plan::GM_SCRATCH);
    char* slab = smem + (size_t)nb * xstride + rsvld_plan::GM_SCRATCH + (KSPLIT ? rsvld_plan::GM_PART : 0) + w * GM_SLAB;
    // this wave's K range: whole steps (the last may be ragged)
    const int kbeg = KSPLIT ? min(w * steps_per_way * KSTEP, K) : 0;
    const int kend = KSPLIT ? min(kbeg + steps_per_way * KSTEP, K) : K;
    // the load of a step: instruction i brings pieces (lane & 31) of rows 2 i + (lane >> 5); where they go in the slab
    const int lrow = lane >> 5, lp = lane & 31;
    // the fragment of chunk m: row lane & 15, piece 4 m + (lane >> 4)
    const int fr = lane & 15, fg = lane >> 4;
    const bool col = fr < nb;                                   // this lane's column of the B operand is an activation row
    const char* xs = smem + (size_t)(col ? fr : 0) * xstride;
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int row0 = (KSPLIT ? blk : blk * GM_WAVES + w) * GM_ROWS;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (KSPLIT || row0 < N) {
            const char* wp[GM_LOADS];
#pragma unroll
            for (int i = 0; i < GM_LOADS; ++i)                  // rows past N re-read the last row, never stored
                wp[i] = Wm + ((int64_t)min(row0 + 2 * i + lrow, N - 1) * K + lp * PIECE) * EB;
            // FULL: a whole step inside the range; else the ragged last one, whose pieces past the range are zeros in both operands
            auto load = [&](u32x4 (&r)[GM_LOADS], int k, auto full) __attribute__((always_inline)) {
                const bool in = decltype(full)::value || k + lp * PIECE < kend;
#pragma unroll
                for (int i = 0; i < GM_LOADS; ++i)
                    r[i] = in ? __builtin_nontemporal_load((const u32x4*)(wp[i] + (size_t)k * EB)) : (u32x4){0u, 0u, 0u, 0u};
            };
            auto step = [&](const u32x4 (&r)[GM_LOADS], int k, auto full) __attribute__((always_inline)) {
                constexpr bool FULL = decltype(full)::value;
#pragma unroll
                for (int i = 0; i < GM_LOADS; ++i) {
                    const int row = 2 * i + lrow;
                    *(u32x4*)(slab + row * GM_STEP_BYTES + ((lp ^ row) << 4)) = r[i];
                }
                __builtin_amdgcn_wave_barrier();                // (no instruction: the slab is this wave's, its LDS operations run in order)
#pragma unroll
                for (int m = 0; m < GM_STEP_BYTES / 64; ++m) {  // chunks of 64 bytes per row: one fragment read each
                    const int kc = k + m * (64 / EB);           // first k of the chunk
                    if (FULL || kc < kend) {                    // (uniform)
                        const u32x4 a = *(const u32x4*)(slab + fr * GM_STEP_BYTES + (((4 * m + fg) ^ fr) << 4));
                        const int kx = kc + fg * PIECE;         // this lane's k: PIECE consecutive elements
                        const bool in = col && (FULL || kx < kend);
                        if constexpr (W8) {
                            u32x4 b0 = {0u, 0u, 0u, 0u}, b1 = {0u, 0u, 0u, 0u};
                            if (in) {
                                b0 = *(const u32x4*)(xs + (size_t)kx * 2);
                                b1 = *(const u32x4*)(xs + (size_t)kx * 2 + 16);
                            }
                            acc = gm_mma<T>(gm_cvt8<T>(a[0], a[1]), __builtin_bit_cast(V8, b0), acc);
                            acc = gm_mma<T>(gm_cvt8<T>(a[2], a[3]), __builtin_bit_cast(V8, b1), acc);
                        } else {
                            u32x4 b0 = {0u, 0u, 0u, 0u};
                            if (in) b0 = *(const u32x4*)(xs + (size_t)kx * 2);
                            acc = gm_mma<T>(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b0), acc);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            };
            // Whole steps with two steps of loads in flight: the next step is requested before this one goes through the slab.  (The
            // prefetch inside the loop is unconditional -- the last one or two steps are peeled -- so that the wait in front of a slab
            // write counts the next step's loads as outstanding instead of draining them.)
            constexpr std::true_type whole{};
            constexpr std::false_type ragged{};
            u32x4 r0[GM_LOADS], r1[GM_LOADS];
            int k = kbeg, n = (kend - kbeg) / KSTEP;
            if (n > 0) {
                load(r0, k, whole);
                for (; n >= 3; n -= 2, k += 2 * KSTEP) {
                    load(r1, k + KSTEP, whole);
                    step(r0, k, whole);
                    load(r0, k + 2 * KSTEP, whole);
                    step(r1, k + KSTEP, whole);
                }
                if (n == 2) {
                    load(r1, k + KSTEP, whole);
                    step(r0, k, whole);
                    step(r1, k + KSTEP, whole);
                    k += 2 * KSTEP;
                } else {
                    step(r0, k, whole);
                    k += KSTEP;
                }
            }
            if (k < kend) {
                load(r0, k, ragged);
                step(r0, k, ragged);
            }
        }
        // D: lane holds rows 4 (lane >> 4) + i of the block, column lane & 15
        if constexpr (KSPLIT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) part[(w * GM_ROWS + 4 * fg + i) * 16 + fr] = acc[i];
            __syncthreads();
            const int r = tid >> 4, c = tid & 15, row = row0 + r;
            if (c < nb && row < N) {                            // fixed order: wave 0 .. 3
                float v = ((part[r * 16 + c] + part[(GM_ROWS + r) * 16 + c]) + part[(2 * GM_ROWS + r) * 16 + c]) + part[(3 * GM_ROWS + r) * 16 + c];
                if constexpr (W8) v = v * scale[row];
                gv_store<T>(y + (size_t)c * N, bias, residual != nullptr ? residual + (size_t)c * N : nullptr, row, v);
            }
            __syncthreads();                                    // the partial sums are rewritten by the next block of rows
        } else {
            if (col) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = row0 + 4 * fg + i;
                    if (row < N) {
                        float v = acc[i];
                        if constexpr (W8) v = v * scale[row];
                        gv_store<T>(y + (size_t)fr * N, bias, residual != nullptr ? residual + (size_t)fr * N : nullptr, row, v);
                    }
                }
            }
        }
    }
}

template <typename T, bool KSPLIT, bool W8>
int gm_go(const rsvld_gemv_mma_plan& pl, const void* w, const float* scale, const void* x, const void* bias, const void* norm_w, float eps,
          const void* residual, int glu, void* y, int N, int K, int nb, hipStream_t s) {
    constexpr auto KERN = gemv_mma_kernel<T, KSPLIT, W8>;
    const int xstride = (int)rsvld_plan::gm_xstride(K);
    const size_t smem = (size_t)nb * xstride + rsvld_plan::GM_SCRATCH + (KSPLIT ? rsvld_plan::GM_PART : 0) + GM_WAVES * GM_SLAB;
    if (smem > (size_t)GVR_LDS) return RSVLD_EUNSUPPORTED;       // (cannot happen: group_rows rows fit)
    if (smem > 65536 && rsvld_smem_once<KERN>(GVR_LDS) != hipSuccess) return RSVLD_ELAUNCH;
    const int per_cu = (int)(GVR_LDS / smem) < 2 ? (int)(GVR_LDS / smem) : 2;     // workgroups a CU holds: LDS, registers (any grid gives the same results)
    const int grid = pl.blocks < GVR_CUS * per_cu ? pl.blocks : GVR_CUS * per_cu;
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(64 * GM_WAVES), smem, s, w, scale, (const T*)x, (const T*)bias, (T*)y, N, K, (const T*)norm_w, eps,
                       (const T*)residual, glu, nb, pl.blocks, xstride, pl.steps_per_way);
    return RSVLD_OK;
}

// The product for B rows, checked (gv_check: the VALU entry points' limits and error codes), in equal groups of at most plan.group_rows
// rows -- a group is one launch and one pass over the weights (K = 14 336: 2 x 4 at B = 8).  B enters nothing but the grouping.
template <bool W8>
int gm_launch(const void* w, const float* scale, const void* x, const void* bias, const void* norm_w, float eps, const void* residual, int glu,
              void* y, int N, int K, int B, int dtype, void* stream) {
    if (const int rc = gv_check<W8>(w, scale, x, norm_w, glu, y, N, K, B, dtype); rc != RSVLD_OK) return rc;
    rsvld_gemv_mma_plan pl;
    if (const int rc = rsvld_plan::plan_gemv_mma(N, K, W8 ? 1 : 0, dtype, &pl); rc != RSVLD_OK) return rc;
    glu = glu ? 1 : 0;
    const int ngroups = (B + pl.group_rows - 1) / pl.group_rows, g = (B + ngroups - 1) / ngroups;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += g) {
        const int nb = B - b0 < g ? B - b0 : g;
        const char* xg = (const char*)x + (size_t)b0 * (glu ? 2 : 1) * K * 2;
        const char* rg = residual ? (const char*)residual + (size_t)b0 * N * 2 : nullptr;
        char* yg = (char*)y + (size_t)b0 * N * 2;
        const int rc = by_dtype(dtype, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            return pl.ksplit ? gm_go<T, true, W8>(pl, w, scale, xg, bias, norm_w, eps, rg, glu, yg, N, K, nb, s)
                             : gm_go<T, false, W8>(pl, w, scale, xg, bias, norm_w, eps, rg, glu, yg, N, K, nb, s);
        });
        if (rc != RSVLD_OK) return rc;
    }
    return rsvld_check_launch();
}

}  // namespace

extern "C" int rsvld_plan_gemv_mma(int N, int K, int w8, int dtype, rsvld_gemv_mma_plan* plan) {
    if (plan == nullptr) return RSVLD_EINVAL;
    return rsvld_plan::plan_gemv_mma(N, K, w8, dtype, plan);
}

extern "C" int rsvld_gemv_mma_rows_fused(const void* w, const void* x, const void* bias, const void* norm_w, float norm_eps, const void* residual,
                                         int glu, void* y, int N, int K, int B, int dtype, void* stream) {
    return gm_launch<false>(w, nullptr, x, bias, norm_w, norm_eps, residual, glu, y, N, K, B, dtype, stream);
}

extern "C" int rsvld_gemv_w8_mma_rows_fused(const void* q, const float* scale, const void* x, const void* bias, const void* norm_w, float norm_eps,
                                            const void* residual, int glu, void* y, int N, int K, int B, int dtype, void* stream) {
    return gm_launch<true>(q, scale, x, bias, norm_w, norm_eps, residual, glu, y, N, K, B, dtype, stream);
}
