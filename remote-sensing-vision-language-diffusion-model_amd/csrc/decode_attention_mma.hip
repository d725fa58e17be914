// decode_attention_mma.hip — the decode step of grouped-query attention over a static cache on MFMAs, head_dim 128, for the B = 1..8
// sequences of the batched token loop (llava_next.FastDecoder(decode_attention="mfma")): the operands, the cache update and the
// partial / combine scheme of da_kernel (gemv.hip), the arithmetic of prefill_attn_d128 (prefill_attention.hip).  Contract:
// include/rsvld_hip.h.
//
//   dam_prologue_kernel  the new token: q and k rotated by da_rope (decode_attention.h, da_kernel's own roundings), k and v into the
//                        caches at the clamped pos[b], the rotated q into the workspace.  One workgroup per (head, sequence).
//   dam_kernel           workgroup = (kv head, range of DAM_RANGE keys on absolute boundaries, sequence); it only reads (stream order
//                        makes the new row visible).  K and V of the range -- two 64-key tiles each, requested at once -- come by LDS-DMA
//                        alone with prefill_attn_d128's source-side XOR swizzles: K read row-wise (ds_read_b128), V through the
//                        hardware transpose.  Wave w takes keys 32 w .. 32 w + 31 of the range: S^T[key][head] on 8 MFMAs, the
//                        group's g query heads on the columns (a padding column repeats head g - 1 and stores nothing), the softmax
//                        of its 32 keys register-local (one exchange with lane ^ 32), P^T rounded to T as the B operand of
//                        O^T[d][head] += V^T P^T on 8 MFMAs.  The waves' (m, l, O) meet in LDS -- over the K tiles, behind a barrier
//                        -- and are folded in wave order; the range's partial leaves in da_kernel's layout for da_combine_kernel.
// Bit-exactness: a key above the position is never requested (its tile row re-reads row pos, which the prologue wrote), its score is
// -inf by SELECTION, its P exactly 0 and its V registers zero; a wave or a range wholly above the position computes nothing (the
// range writes the neutral partial m = -inf, l = 0, O = 0).  Nothing here knows B or another sequence; max_len enters addresses only.
#include "rsvld_common.h"
#include "rsvld_plan.h"
#include "decode_attention.h"

namespace {

using rsvld_plan::DAM_RANGE;
typedef short s16x8 __attribute__((__vector_size__(8 * sizeof(short))));
constexpr int DAM_TILE = 64 * 256;   // 64 keys x 128 d, 16-bit
constexpr int DAM_PSTRIDE = DA_PART + 2;   // floats between the partials of two heads in LDS: 16-byte aligned rows
static_assert(4 * DAM_TILE == rsvld_plan::DAM_LDS_BYTES && 4 * DA_GMAX * DAM_PSTRIDE * 4 <= 2 * DAM_TILE, "the waves' partials fit over the K tiles");

template <typename T>
__global__ __launch_bounds__(DA_HD) void dam_prologue_kernel(const T* __restrict__ qkv, const T* __restrict__ cosv, const T* __restrict__ sinv,
                                                             const long long* __restrict__ pos_p, T* __restrict__ kc, T* __restrict__ vc,
                                                             T* __restrict__ qrot, int n_q, int n_kv, int max_len) {
    const int h = blockIdx.x, d = threadIdx.x, half = DA_HD / 2;
    const size_t seq = blockIdx.y;
    qkv += seq * (size_t)(n_q + 2 * n_kv) * DA_HD;
    cosv += seq * DA_HD;
    sinv += seq * DA_HD;
    if (h < n_q) {
        qrot[(seq * n_q + h) * DA_HD + d] = (T)da_rope(qkv + (size_t)h * DA_HD, cosv, sinv, half, d);
    } else {
        const int kvh = h - n_q, p = (int)min(max(pos_p[seq], 0ll), (long long)max_len - 1);   // (clamped, never written past the cache)
        const size_t row = ((seq * n_kv + kvh) * (size_t)max_len + p) * DA_HD;
        kc[row + d] = (T)da_rope(qkv + (size_t)(n_q + kvh) * DA_HD, cosv, sinv, half, d);
        vc[row + d] = qkv[(size_t)(n_q + n_kv + kvh) * DA_HD + d];
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void dam_kernel(const T* __restrict__ qrot, const long long* __restrict__ pos_p, const T* __restrict__ kc,
                                                     const T* __restrict__ vc, float* __restrict__ ws, int n_q, int n_kv, int max_len,
                                                     float scale) {
    constexpr int D = DA_HD;
    typedef typename Mfma<T>::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[4 * DAM_TILE];   // K[2] | V[2]; after the products the waves' partials over K
    const int kvh = blockIdx.x, c = blockIdx.y, nr = gridDim.y;
    const size_t seq = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int G = n_q / n_kv, p = (int)min(max(pos_p[seq], 0ll), (long long)max_len - 1);
    float* out = ws + seq * (size_t)n_q * nr * DA_PART + ((size_t)(kvh * nr + c) * G) * DA_PART;
    const int j0 = c * DAM_RANGE;
    if (j0 > p) {                                                      // (workgroup-uniform) nothing of this range is visible yet
        for (int i = tid; i < G * DA_PART; i += 256) out[i] = (i % DA_PART) == DA_HD ? -INFINITY : 0.f;
        return;
    }
    const T* Kb = kc + (seq * n_kv + kvh) * (size_t)max_len * D;
    const T* Vb = vc + (seq * n_kv + kvh) * (size_t)max_len * D;

    // ---- both tiles, requested at once.  Wave w moves key rows 16 w .. 16 w + 15 of a tile, as in prefill_attn_d128: lane (row = lane >> 4,
    // pos = lane & 15) of piece i fills LDS chunk `pos` of tile row r = 16 w + 4 i + row with source chunk pos ^ (r & 15) for K and
    // pos ^ ((r & 3) << 2) for V.  A tile wholly above p is not requested (and not read: its waves are off).
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k0 = j0 + t * 64;
        if (k0 > p) break;
        const uint32_t kd = lds0 + t * DAM_TILE + wu * 4096, vd = kd + 2 * DAM_TILE;
        if (k0 + 63 <= p) {
            const char* kb = (const char*)(Kb + (size_t)(k0 + wu * 16) * D);
            const char* vb = (const char*)(Vb + (size_t)(k0 + wu * 16) * D);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * i + (lane >> 4);
                rsvld_lds_dma16(kb, (uint32_t)(rr * 256) + (uint32_t)(((lane & 15) ^ rr) << 4), kd + i * 1024);
                rsvld_lds_dma16(vb, (uint32_t)(rr * 256) + (uint32_t)(((lane & 15) ^ ((rr & 3) << 2)) << 4), vd + i * 1024);
            }
        } else {   // rows above p re-read row p (< max_len, written by the prologue); their scores are masked and their V rows zeroed
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * i + (lane >> 4);
                const int key = min(k0 + wu * 16 + rr, p);
                rsvld_lds_dma16_addr((const char*)(Kb + (size_t)key * D) + (((lane & 15) ^ rr) << 4), kd + i * 1024);
                rsvld_lds_dma16_addr((const char*)(Vb + (size_t)key * D) + (((lane & 15) ^ ((rr & 3) << 2)) << 4), vd + i * 1024);
            }
        }
    }

    // ---- Q fragments (B operand: col = the head on the lane, k = d); a padding column repeats the group's last head
    const int hq = kvh * G + min(l31, G - 1);
    const T* Qr = qrot + (seq * n_q + hq) * D;
    v8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = __builtin_bit_cast(v8, *(const u32x4*)(Qr + ks * 16 + lh * 8));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // the tiles landed

    // wave w: keys kw0 .. kw0 + 31 = rows 32 (w & 1) .. of tile w >> 1
    const int kw0 = j0 + 32 * w;
    const bool wave_on = kw0 <= p;                                     // (wave-uniform)
    f32x16 oacc[4];
    float m_w = -INFINITY, l_w = 0.f;
    if (wave_on) {
        const int tile = w >> 1, kt = w & 1;
        const char* Ks = smem + tile * DAM_TILE + kt * 8192;
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const v8 kf = *(const v8*)(Ks + l31 * 256 + (((2 * ks + lh) ^ (l31 & 15)) << 4));
            sacc = Mfma<T>::mma(kf, qf[ks], sacc);
        }
        // ---- scale in fp32; the keys above p by selection (a NaN score of such a key never enters the arithmetic)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] *= scale;
        const bool edge = kw0 + 31 > p;                                // (wave-uniform)
        if (edge) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kw0 + (r & 3) + 8 * (r >> 2) + 4 * lh > p) sacc[r] = -INFINITY;
        }
        // ---- softmax of the wave's 32 keys (this lane: 16 of its head's scores, lane ^ 32 the rest); key kw0 <= p is unmasked
        float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int r = 0; r < 16; ++r) m4[r >> 2] = fmaxf(m4[r >> 2], sacc[r]);
        float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        m_w = fmaxf(mx, __shfl_xor(mx, 32));
        float r4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = __expf(sacc[r] - m_w);
            sacc[r] = pv;
            r4[r >> 2] += pv;
        }
        l_w = (r4[0] + r4[1]) + (r4[2] + r4[3]);
        l_w += __shfl_xor(l_w, 32);
        v8 pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[s][j] = (T)sacc[8 * s + j];
        // ---- O^T[d][head] = V^T P^T.  A operand (row = d, k = key in P's register order): lane 16 g1 + 4 qq + pp supplies row
        // 16 s4 + 8 hf + 4 lh + qq of the tile, d = 32 dt + 16 (g1 & 1) + 4 pp .. + 3 (prefill_attn_d128's transposed read)
        const int qq = (lane >> 2) & 3, pp = lane & 3, g1 = (lane >> 4) & 1;
        const int vbase = 2 * DAM_TILE + tile * DAM_TILE + (4 * lh + qq) * 256 + ((2 * g1 + (pp >> 1)) << 4) + ((pp & 1) << 3);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int off = vbase + ((dt ^ qq) << 6) + (2 * kt + s) * 4096;
                s16x8 vv = tr16_pair<s16x8>(lds_read_tr16(smem + off), lds_read_tr16(smem + off + 2048));
                if (edge) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (kw0 + 16 * s + 8 * (j >> 2) + 4 * lh + (j & 3) > p) vv[j] = 0;
                }
                oacc[dt] = Mfma<T>::mma(__builtin_bit_cast(v8, vv), pf[s], oacc[dt]);
            }
    }
    __syncthreads();   // every wave is done with the K and V tiles

    // ---- the waves' partials: part[w][head][DAM_PSTRIDE] over the K tiles; d = 32 dt + 8 (r >> 2) + 4 lh + (r & 3) on head l31
    float* part = (float*)smem;
    if (wave_on && l31 < G) {
        float* o = part + (w * DA_GMAX + l31) * DAM_PSTRIDE;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg)
                *(f32x4*)(o + dt * 32 + 8 * gg + 4 * lh) = (f32x4){oacc[dt][4 * gg], oacc[dt][4 * gg + 1], oacc[dt][4 * gg + 2], oacc[dt][4 * gg + 3]};
        if (lh == 0) { o[DA_HD] = m_w; o[DA_HD + 1] = l_w; }
    }
    __syncthreads();
    // ---- folded in wave order: the waves that hold a key (0 .. nw - 1; wave 0 always does)
    const int nw = min(4, (p - j0) / 32 + 1);
    for (int i = tid; i < G * DA_HD; i += 256) {
        const int g = i / DA_HD, d = i % DA_HD;
        const float* o = part + g * DAM_PSTRIDE;
        float M = o[DA_HD];
        for (int ww = 1; ww < nw; ++ww) M = fmaxf(M, o[ww * DA_GMAX * DAM_PSTRIDE + DA_HD]);
        float acc = 0.f, l = 0.f;
        for (int ww = 0; ww < nw; ++ww) {
            const float* ow = o + ww * DA_GMAX * DAM_PSTRIDE;
            const float e = __expf(ow[DA_HD] - M);
            acc = __builtin_fmaf(e, ow[d], acc);
            l = __builtin_fmaf(e, ow[DA_HD + 1], l);
        }
        out[g * DA_PART + d] = acc;
        if (d == 0) { out[g * DA_PART + DA_HD] = M; out[g * DA_PART + DA_HD + 1] = l; }
    }
}

template <typename T>
void dam_launch(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache, void* vcache, void* out, float* ws,
                int n_q, int n_kv, int max_len, int B, float scale, int dtype, int ranges, hipStream_t s) {
    T* qrot = (T*)ws;                                                   // [B][n_q][128] in T = B n_q 64 floats, then the partials
    float* part = ws + (size_t)B * n_q * (DA_HD / 2);
    hipLaunchKernelGGL((dam_prologue_kernel<T>), dim3(n_q + n_kv, B), dim3(DA_HD), 0, s, (const T*)qkv, (const T*)cosv, (const T*)sinv,
                       (const long long*)pos, (T*)kcache, (T*)vcache, qrot, n_q, n_kv, max_len);
    hipLaunchKernelGGL((dam_kernel<T>), dim3(n_kv, ranges, B), dim3(256), 0, s, (const T*)qrot, (const long long*)pos, (const T*)kcache,
                       (const T*)vcache, part, n_q, n_kv, max_len, scale);
    rsvld_da_combine_launch(part, out, n_q, n_kv, ranges, B, dtype, s);
}

}  // namespace

extern "C" int rsvld_plan_llama_decode_attention_mma(int n_q, int n_kv, int max_len, int dtype, rsvld_decode_attention_mma_plan* plan) {
    if (plan == nullptr) return RSVLD_EINVAL;
    return rsvld_plan::plan_decode_attention_mma(n_q, n_kv, max_len, dtype, plan);
}

extern "C" size_t rsvld_llama_decode_attention_mma_rows_ws_bytes(int n_q, int n_kv, int max_len, int B) {
    if (n_q <= 0 || n_kv <= 0 || max_len <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return 0;
    const size_t ranges = ((size_t)max_len + DAM_RANGE - 1) / DAM_RANGE;
    return (size_t)B * n_q * (DA_HD / 2 + ranges * DA_PART) * sizeof(float);
}

extern "C" int rsvld_llama_decode_attention_mma_rows(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache,
                                                     void* vcache, void* out, float* ws, int n_q, int n_kv, int head_dim, int max_len, int B,
                                                     float scale, int dtype, void* stream) {
    if (!qkv || !cosv || !sinv || !pos || !kcache || !vcache || !out || !ws) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (n_q <= 0 || n_kv <= 0 || max_len <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return RSVLD_EINVAL;
    if (head_dim != DA_HD) return RSVLD_EUNSUPPORTED;
    rsvld_decode_attention_mma_plan pl;
    const int rc = rsvld_plan::plan_decode_attention_mma(n_q, n_kv, max_len, dtype, &pl);
    if (rc != RSVLD_OK) return rc;
    if (((uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)qkv | (uintptr_t)ws) & 15) return RSVLD_EINVAL;
    if (dtype == RSVLD_F16)
        dam_launch<f16>(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, scale, dtype, pl.ranges, (hipStream_t)stream);
    else
        dam_launch<bf16>(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, scale, dtype, pl.ranges, (hipStream_t)stream);
    return rsvld_check_launch();
}
