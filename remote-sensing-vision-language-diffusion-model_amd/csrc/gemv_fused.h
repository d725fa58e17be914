// gemv_fused.h -- what the two families of decode products share (gemv.hip: the VALU kernels; gemv_mma.hip: the MFMA kernels): the staging
// of an activation row with its fused neighbours (gv_stage_x), the epilogue (gv_store) and the operand checks of the entry points
// (gv_check).  ONE statement of these roundings and limits: the staged row x' and the epilogue are the same bits in both families.
// Included inside each unit's anonymous namespace.
#pragma once

constexpr int GV_WAVES = 4;    // waves per workgroup
constexpr int GV_RPW = 4;      // rows a wave of the VALU kernels accumulates at a time

// Fused forms (round 5, rsvld_gemv_fused: the decode step of a Llama layer in five launches instead of ~26 small ones).  All three act on
// the activation row while it is staged into LDS, or on the result before its one store -- outside the weight-streaming loop:
//   norm_w != nullptr   x <- T( x * rsqrt(mean(x^2) + eps) * norm_w )         (the RMSNorm in front of q|k|v, gate|up and lm_head)
//   glu                 x has 2 K elements [gate | up]: x <- T( T(silu(gate)) * up )   (the SwiGLU in front of down_proj)
//   residual != nullptr y <- T( residual + T(W x + b) )                        (h + o_proj(...), h + down_proj(...))
// with the roundings of the unfused torch sequence (F.rms_norm, silu(g) * u, h + linear) kept where they were.  gv_stage_x / gv_store are
// shared by the 16-bit kernel and the e4m3 one (gemv_w8_kernel): one statement of these roundings.
// gv_stage_x: the activation row into LDS as K elements of T (4 floats of reduction scratch ``red_off`` bytes behind it), closed by a barrier.
// (Thread indices come from the kernel and the pointers carry no __restrict__: in this form the 16-bit kernels' weight-streaming loops and
// epilogues compile to the instructions they had with the staging written out in the kernel -- only address arithmetic of the staging itself
// is ordered differently -- and they time the same; with __restrict__ parameters the row route measured 1 % slower.)
template <typename T>
__device__ __forceinline__ void gv_stage_x(char* smem, int red_off, const T* x, const T* norm_w, float eps, int K, int glu,
                                           const int tid, const int lane, const int w) {
    if (glu) {
        for (int i = tid * 8; i < K; i += 64 * GV_WAVES * 8) {
            float g[8], u[8];
            unpack8<T>(*(const u32x4*)(x + i), g);
            unpack8<T>(*(const u32x4*)(x + K + i), u);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
#pragma clang fp contract(off)
                const T sg = (T)silu_f(g[e]);     // (silu rounded, THEN the product: two torch kernels)
                g[e] = (float)sg * u[e];
            }
            *(u32x4*)(smem + i * 2) = pack8<T>(g);
        }
    } else if (norm_w != nullptr) {
        float* red = (float*)(smem + (size_t)K * 2 + red_off);
        float ss = 0.f;
        for (int i = tid * 8; i < K; i += 64 * GV_WAVES * 8) {
            float f[8];
            unpack8<T>(*(const u32x4*)(x + i), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(f[e], f[e], ss);
        }
        ss = wave_sum(ss);
        if (lane == 0) red[w] = ss;
        __syncthreads();
        const float inv = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + eps);
        for (int i = tid * 8; i < K; i += 64 * GV_WAVES * 8) {
            float f[8], g[8];
            unpack8<T>(*(const u32x4*)(x + i), f);
            unpack8<T>(*(const u32x4*)(norm_w + i), g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = f[e] * inv * g[e];
            *(u32x4*)(smem + i * 2) = pack8<T>(f);
        }
    } else {
        for (int i = tid * 8; i < K; i += 64 * GV_WAVES * 8) *(u32x4*)(smem + i * 2) = *(const u32x4*)(x + i);
    }
    __syncthreads();
}
// gv_store: y[row] = T(v + bias[row]), then the residual
template <typename T>
__device__ __forceinline__ void gv_store(T* y, const T* bias, const T* residual, int row, float v) {
    T r = (T)(v + (bias != nullptr ? (float)bias[row] : 0.f));
    if (residual != nullptr) r = (T)((float)residual[row] + (float)r);
    y[row] = r;
}

constexpr int GVR_LDS = 160 * 1024;     // LDS of a CU: what one workgroup may hold (registered per kernel above 64 KiB)
constexpr int GVR_CUS = 256;            // sizes the persistent grid only (any grid gives the same results)
// dynamic LDS of a VALU launch with nb staged rows (the kernels' layout)
constexpr size_t gv_lds_bytes(int K, int nb, bool ksplit) {
    return (size_t)nb * K * 2 + (ksplit ? nb * 4 * GV_RPW * sizeof(float) : 0) + 16 * sizeof(float);
}

// the element type of RSVLD_F16 / RSVLD_BF16 (checked by the caller), resolved once: f gets a null T* to name T by
template <typename F> auto by_dtype(int dtype, F&& f) { return dtype == RSVLD_F16 ? f((f16*)nullptr) : f((bf16*)nullptr); }

// The operands of a product, for all the entry points of both families.  W8: pieces of 16 weights (K % 16) and a scale per row; else
// pieces of 8 (K % 8).
// ONE row with its K-split partial sums must fit the 64 KiB of dynamic LDS a launch gets without an opt-in (more rows go in groups).
// (glu reads x[b] + K as 16-byte pieces too: aligned because x is and K % 8 == 0 makes K * 2 bytes a multiple of 16 -- no check of its own.)
template <bool W8>
int gv_check(const void* w, const float* scale, const void* x, const void* norm_w, int glu, const void* y, int N, int K, int B, int dtype) {
    if (!w || (W8 && !scale) || !x || !y || N <= 0 || K <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (K % (W8 ? 16 : 8) != 0 || gv_lds_bytes(K, 1, true) > 65536) return RSVLD_EUNSUPPORTED;
    if ((((uintptr_t)w | (uintptr_t)x | (uintptr_t)norm_w) & 15) || (W8 && ((uintptr_t)scale & 3))) return RSVLD_EINVAL;
    if (glu && norm_w != nullptr) return RSVLD_EINVAL;
    return RSVLD_OK;
}
