// decode_attention.h — what the two decode-step attentions (da_kernel of gemv.hip, the MFMA form of decode_attention_mma.hip) share: the
// rotary embedding of the new token, so that both leave the same bits in the caches, the layout of the partials and the host
// launch of da_combine_kernel, which folds the partials of either.
#pragma once
#include "rsvld_common.h"

constexpr int DA_HD = 128, DA_GMAX = 8;
constexpr int DA_PART = DA_HD + 2;   // floats of one partial: O[128] | m | l.  Workspace: [sequence][kv head][chunk][head in group][DA_PART]

// rotary embedding as the unfused sequence rounds it: T(x cos) + T(rot(x) sin) -> T
template <typename T>
__device__ __forceinline__ float da_rope(const T* src, const T* cosv, const T* sinv, int half, int i) {
#pragma clang fp contract(off)   // (three roundings, as three torch kernels leave them: hipcc otherwise demotes the sum to ONE 16-bit fma)
    const float xr = i < half ? -(float)src[i + half] : (float)src[i - half];
    const T a = (T)((float)src[i] * (float)cosv[i]);
    const T b = (T)(xr * (float)sinv[i]);
    return (float)(T)((float)a + (float)b);
}

// da_combine_kernel (gemv.hip) on partials ws [B][n_q x nchunk x DA_PART] -> out [B][n_q x 128]; dtype RSVLD_F16 / RSVLD_BF16
void rsvld_da_combine_launch(const float* ws, void* out, int n_q, int n_kv, int nchunk, int B, int dtype, hipStream_t stream);
