// prefill_attention.hip — causal grouped-query flash attention over one sequence's static cache, head_dim 128: the attention of the
// caption pass's PREFILL (llava_next.FastDecoder(prefill="flash")).  The score matrix never exists in memory, only the filled prefix of
// the cache is read, and a query row's result does not depend on what surrounds it (the contract in include/rsvld_hip.h).
//
// House style of attention.hip's attn_d64b: S^T = K Q^T "swapped" (keys on the accumulator registers, the query row on the lane), so the
// online softmax is register-local (one exchange with lane ^ 32) and the converted score tile is the B operand of O^T += V^T P^T in
// place; K and V tiles of 64 keys go through a double-buffered LDS ring filled by LDS-DMA alone, K is read row-wise (ds_read_b128), V
// through the hardware transpose (ds_read_b64_tr_b16), both images XOR-swizzled on the DMA's source side; one barrier per tile.  The
// tile layout, its swizzles, the Q fragments and the register -> key map are attention_d128.h's, shared with the decode step (dam_kernel);
// the tile walk, the double buffering and the online softmax (exp2) are this kernel's.  What is different from attn_d64b:
//   * rows are (position, head-in-group) pairs of ONE kv head in the [T g] order FastDecoder.forward forms: row r = t g + j is query head
//     kvh g + j at position pos0 + t.  A workgroup (4 waves x 32 rows) owns 128 such rows, so one K / V tile serves all g query heads;
//   * causal: a workgroup walks key tiles 0 .. (its last position) / 64 in ascending order on absolute 64-key boundaries, a wave skips
//     the tiles wholly above its own last position and masks only the tiles that reach above its first;
//   * the scores stay fp32 (scaled in fp32, never rounded to 16 bits); P is rounded to the 16-bit type only as the PV operand;
//   * the MFMAs are the compiler's builtins (it pads the hazards), a plain online softmax: no bias step, no deferred rescale.
// Bit-exactness: a masked score is -inf by SELECTION, its P is exactly 0, and a tile that holds no key of a row leaves that row's
// (m, l, O) exactly as they were (alpha = exp2(0) = 1, + 0).  V rows above the wave's last position are replaced by zeros in the
// fragment registers (0 x NaN would be NaN) and K / V rows above the call's last position are never even requested.
#include "rsvld_common.h"
#include "rsvld_plan.h"
#include "attention_d128.h"

namespace {

struct PrefillArgs {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    int64_t q_ts;      // elements between the q rows of consecutive tokens
    int T, pos0, n_q, g, max_len;
    float scale_log2e;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void prefill_attn_d128_kernel(PrefillArgs p) {
    constexpr int D = 128;
    typedef typename Mfma<T>::v8 v8;
    typedef typename Mfma<T>::v4 v4;
    __shared__ __attribute__((aligned(16))) char smem[4 * A128_TILE];   // K[2] | V[2]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int g = p.g, kvh = blockIdx.y;
    const int R = p.T * g;                                            // rows of this kv head
    // longest key ranges first: block 0 owns the LAST rows
    const int rb = (int)gridDim.x - 1 - (int)blockIdx.x;
    const int wg_last = min(R - 1, rb * 128 + 127) / g;               // (token index of) the workgroup's last position
    const int nt = ((p.pos0 + wg_last) >> 6) + 1;                     // key tiles 0 .. nt - 1
    const int klast = p.pos0 + p.T - 1;                               // the last key of the call: nothing above it is requested
    const int r0 = rb * 128 + w * 32;                                 // this wave's rows r0 .. r0 + 31
    const bool wave_on = r0 < R;                                      // (a wave of padding rows only moves tiles)
    const int p_min = p.pos0 + min(r0, R - 1) / g, p_max = p.pos0 + min(r0 + 31, R - 1) / g;
    const int row = min(r0 + l31, R - 1);                             // a padding lane repeats the last row and stores nothing
    const int tq = row / g, hq = kvh * g + (row - tq * g);
    const int my_pos = p.pos0 + tq;
    const T* Kb = (const T*)p.k + (int64_t)kvh * p.max_len * D;
    const T* Vb = (const T*)p.v + (int64_t)kvh * p.max_len * D;

    // ---- tile DMA (attention_d128.h): tile t goes to buffer t & 1; nothing above klast is requested
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
    uint32_t kvo[4], vvo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rr = 4 * i + (lane >> 4);
        kvo[i] = (uint32_t)(rr * 256) + (uint32_t)a128_k_swz(lane, rr);
        vvo[i] = (uint32_t)(rr * 256) + (uint32_t)a128_v_swz(lane, rr);
    }
    auto dma_tile = [&](int t) {
        const int buf = t & 1;
        const uint32_t kd = lds0 + buf * A128_TILE + wu * 4096, vd = kd + 2 * A128_TILE;
        if (t * 64 + 63 <= klast) {
            const char* kb = (const char*)(Kb + (int64_t)(t * 64 + wu * 16) * D);
            const char* vb = (const char*)(Vb + (int64_t)(t * 64 + wu * 16) * D);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rsvld_lds_dma16(kb, kvo[i], kd + i * 1024);
                rsvld_lds_dma16(vb, vvo[i], vd + i * 1024);
            }
        } else {   // rows above klast re-read key klast (< max_len)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * i + (lane >> 4);
                const int key = min(t * 64 + wu * 16 + rr, klast);
                rsvld_lds_dma16_addr((const char*)(Kb + (int64_t)key * D) + a128_k_swz(lane, rr), kd + i * 1024);
                rsvld_lds_dma16_addr((const char*)(Vb + (int64_t)key * D) + a128_v_swz(lane, rr), vd + i * 1024);
            }
        }
    };
    dma_tile(0);

    // ---- Q fragments (B operand: col = the row on the lane, k = d)
    const T* Qr = (const T*)p.q + (int64_t)tq * p.q_ts + (int64_t)hq * D;
    v8 qf[8];
    a128_load_q<T>(Qr, lh, qf);
    f32x16 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;   // (tile 0 holds key 0, which every row attends: m_run is finite from there on)

    // per-lane read offsets, kept over the loop: K of row kt 32 + l31, V of the 16-key group s4 at + s4 * 4096
    int koff[8], voff[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = a128_k_off(l31, lh, ks);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {   // V (attention_d128.h: the transposed read)
        const int qq = (lane >> 2) & 3, pp = lane & 3, g1 = (lane >> 4) & 1;
        voff[dt] = 2 * A128_TILE + (4 * lh + qq) * 256 + ((dt ^ qq) << 6) + ((2 * g1 + (pp >> 1)) << 4) + ((pp & 1) << 3);
    }

    a128_pin_q(qf);    // (the wait for the Q loads stays out of the loop)
    __syncthreads();   // tile 0 landed

    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        // tile t + 1 goes to the buffer tile t - 1 was read from, i.e. before the last barrier
        if (t + 1 < nt) dma_tile(t + 1);
        if (wave_on && t * 64 <= p_max) {   // (wave-uniform) else: every key of the tile lies above every row of this wave
            const char* Ks = smem + buf * A128_TILE;
            const int vb = buf * A128_TILE;
            // ---- S^T[key][row]: two 32-key halves x 8 k-steps
            f32x16 sacc[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const v8 kf = *(const v8*)(Ks + kt * 8192 + koff[ks]);
                    sacc[kt] = Mfma<T>::mma(kf, qf[ks], sacc[kt]);
                }
            }
            // ---- scale in fp32, causal mask on the tiles that reach above the wave's first position (by selection: a NaN score of a
            // key above the row's position never enters the arithmetic)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kt][r] *= p.scale_log2e;
            const bool diag = t * 64 + 63 > p_min;
            if (diag) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (t * 64 + kt * 32 + a128_key(r, lh) > my_pos) sacc[kt][r] = -INFINITY;
                    }
            }
            // ---- online softmax, register-local (this lane: 32 of its row's 64 scores, lane ^ 32 the rest)
            float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) m4[r >> 2] = fmaxf(m4[r >> 2], sacc[kt][r]);
            float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);                     // finite: see m_run
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // exp2(-inf) = 0 on tile 0, exp2(0) = 1 where the maximum stays
            m_run = m_new;
            float r4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(sacc[kt][r] - m_new);
                    sacc[kt][r] = pv;
                    r4[r >> 2] += pv;
                }
            l_run = l_run * alpha + ((r4[0] + r4[1]) + (r4[2] + r4[3]));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            v8 pf[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[s4][j] = (T)sacc[s4 >> 1][8 * (s4 & 1) + j];
            // ---- O^T[d][row] += V^T P^T
            const bool vclean = t * 64 + 63 > p_max;   // (wave-uniform) the tile holds keys above every row of this wave: their V rows -> 0
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int off = vb + voff[dt] + s4 * 4096;
                    s16x8 vv = tr16_pair<s16x8>(lds_read_tr16(smem + off), lds_read_tr16(smem + off + 2048));
                    if (vclean) {   // (in place, not in a function of attention_d128.h: see there)
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (t * 64 + 16 * s4 + 8 * (j >> 2) + 4 * lh + (j & 3) > p_max) vv[j] = 0;
                    }
                    oacc[dt] = Mfma<T>::mma(__builtin_bit_cast(v8, vv), pf[s4], oacc[dt]);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t + 1 has landed
        __syncthreads();                                    // everyone is done with buffer t & 1
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    if (r0 + l31 >= R) return;
    const float inv = 1.0f / l_tot;
    T* Ob = (T*)p.out + ((int64_t)tq * p.n_q + hq) * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            v4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (T)(oacc[dt][4 * gg + e] * inv);
            *(v4*)(Ob + dt * 32 + 8 * gg + 4 * lh) = o;
        }
}

}  // namespace

extern "C" int rsvld_plan_llama_prefill_attention(int T, int n_q, int n_kv, int head_dim, rsvld_prefill_attention_plan* plan) {
    if (plan == nullptr) return RSVLD_EINVAL;
    return rsvld_plan::plan_prefill_attention(T, n_q, n_kv, head_dim, plan);
}

extern "C" int rsvld_llama_prefill_attention(const void* q, int64_t q_tok_stride, const void* kcache, const void* vcache, void* out, int T,
                                             int pos0, int n_q, int n_kv, int head_dim, int max_len, float scale, int dtype, void* stream) {
    if (!q || !kcache || !vcache || !out) return RSVLD_EINVAL;
    if (T < 1 || pos0 < 0 || max_len < 1 || (int64_t)pos0 + T > max_len || n_q < 1 || n_kv < 1 || n_q % n_kv != 0) return RSVLD_EINVAL;
    // 16-byte vector access along d
    if ((((uintptr_t)q | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out) & 15) || (q_tok_stride & 7) || q_tok_stride < 0) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EUNSUPPORTED;
    rsvld_prefill_attention_plan pl;
    const int rc = rsvld_plan::plan_prefill_attention(T, n_q, n_kv, head_dim, &pl);
    if (rc != RSVLD_OK) return rc;
    if (T > 1 && q_tok_stride < (int64_t)n_q * head_dim) return RSVLD_EINVAL;   // overlapping token rows
    PrefillArgs a;
    a.q = q; a.k = kcache; a.v = vcache; a.out = out;
    a.q_ts = q_tok_stride;
    a.T = T; a.pos0 = pos0; a.n_q = n_q; a.g = n_q / n_kv; a.max_len = max_len;
    a.scale_log2e = scale * 1.4426950408889634f;
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
    if (dtype == RSVLD_F16)
        hipLaunchKernelGGL(prefill_attn_d128_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(prefill_attn_d128_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return rsvld_check_launch();
}
