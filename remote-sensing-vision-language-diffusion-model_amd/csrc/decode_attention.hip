// decode_attention.hip -- one decode step of grouped-query attention over a static key / value cache, head_dim 128, for the B = 1..8
// sequences of the token loop: rotary embedding of the new q and k (half-split form), the cache write at the clamped pos[b], scores,
// softmax and P V for the G = n_q / n_kv <= 8 query heads that share a kv head.  pos is read from DEVICE memory (the step is replayed from
// a hipGraph).  Two forms, one layout of partials ([sequence][kv head][chunk][head in group][DA_PART], folded by da_combine_kernel) and one
// rotary embedding (da_rope), so that both leave the same bits in the caches.  Contract: include/rsvld_hip.h.
//
// The VALU form (rsvld_llama_decode_attention{,_rows}; llava_next.FastDecoder(decode_attention="valu")):
//   da_kernel            workgroup = (kv head, chunk of DA_CH keys, sequence): every thread requests its pieces of the chunk's K and V rows
//                        FIRST (the cache of a 32-layer decoder does not stay in L2 between steps: one memory latency per launch, not one
//                        per key), the rows go to LDS, then scores, chunk maximum / exponentials / sum per head and the partial output
//                        [G][128] with its (m, l) into the workspace.  Chunks beyond the position write l = 0.
//   da_combine_kernel    folds the chunks of one query head.
// The MFMA form (rsvld_llama_decode_attention_mma_rows; FastDecoder(decode_attention="mfma")), on the K / V tile layout of attention_d128.h:
//   dam_prologue_kernel  the new token: q and k rotated by da_rope, k and v into the caches at the clamped pos[b], the rotated q into the
//                        workspace.  One workgroup per (head, sequence).
//   dam_kernel           workgroup = (kv head, range of DAM_RANGE keys on absolute boundaries, sequence); it only reads (stream order
//                        makes the new row visible).  K and V of the range -- two 64-key tiles each, requested at once -- come by LDS-DMA
//                        alone.  Wave w takes keys 32 w .. 32 w + 31 of the range: S^T[key][head] on 8 MFMAs, the
//                        group's g query heads on the columns (a padding column repeats head g - 1 and stores nothing), the softmax
//                        of its 32 keys register-local (one exchange with lane ^ 32), P^T rounded to T as the B operand of
//                        O^T[d][head] += V^T P^T on 8 MFMAs.  The waves' (m, l, O) meet in LDS -- over the K tiles, behind a barrier
//                        -- and are folded in wave order; the range's partial leaves in da_kernel's layout for da_combine_kernel.
// Bit-exactness of the MFMA form: a key above the position is never requested (its tile row re-reads row pos, which the prologue wrote),
// its score is -inf by SELECTION, its P exactly 0 and its V registers zero; a wave or a range wholly above the position computes nothing
// (the range writes the neutral partial m = -inf, l = 0, O = 0).  Nothing here knows B or another sequence; max_len enters addresses only.
#include "rsvld_common.h"
#include "rsvld_plan.h"
#include "attention_d128.h"
#include <type_traits>   // std::integral_constant (da_row16_sum)

namespace {

constexpr int DA_HD = 128, DA_GMAX = 8;
constexpr int DA_PART = DA_HD + 2;   // floats of one partial: O[128] | m | l

// rotary embedding as the unfused sequence rounds it: T(x cos) + T(rot(x) sin) -> T
template <typename T>
__device__ __forceinline__ float da_rope(const T* src, const T* cosv, const T* sinv, int half, int i) {
#pragma clang fp contract(off)   // (three roundings, as three torch kernels leave them: hipcc otherwise demotes the sum to ONE 16-bit fma)
    const float xr = i < half ? -(float)src[i + half] : (float)src[i - half];
    const T a = (T)((float)src[i] * (float)cosv[i]);
    const T b = (T)(xr * (float)sinv[i]);
    return (float)(T)((float)a + (float)b);
}

// ==== the VALU form
constexpr int DA_CH = 128;   // keys per workgroup: 8 kv heads x 26 chunks = 208 workgroups at the caption's ~3 300 keys
constexpr int DA_ROW = DA_HD * 2 + 16;                 // LDS row stride in bytes: four rows read by one wave instruction fall into different banks
constexpr int DA_PIECES = DA_CH * 16 / 256;            // 16-byte pieces of the K (and of the V) chunk per thread

// sum over the 16 lanes of a DPP row, in every lane: four cross-lane VALU steps (quad swaps, half-row and row mirrors) where
// __shfl_xor would be four dependent ds_bpermute round trips -- 16 of them per key group and wave made the score phase the kernel's longest
__device__ __forceinline__ float da_row16_sum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});     // quad_perm [1, 0, 3, 2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});     // quad_perm [2, 3, 0, 1]
    v += dpp(v, std::integral_constant<int, 0x141>{});    // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});    // row_mirror
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void da_kernel(const T* __restrict__ qkv, const T* __restrict__ cosv, const T* __restrict__ sinv,
                                                 const long long* __restrict__ pos_p, T* __restrict__ kc, T* __restrict__ vc,
                                                 float* __restrict__ ws, int n_q, int n_kv, int max_len, float scale) {
    __shared__ __attribute__((aligned(16))) char ks[DA_CH * DA_ROW], vs[DA_CH * DA_ROW];
    __shared__ float qs[DA_GMAX][DA_HD];        // rotated queries of this kv head's group
    __shared__ float sc[DA_GMAX][DA_CH];        // scores, then exp(s - m)
    __shared__ float ml[DA_GMAX][2];
    const int kvh = blockIdx.x, c = blockIdx.y, nchunk = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // blockIdx.z: the sequence (rsvld_llama_decode_attention_rows; one sequence = the single entry point).  Every operand of a sequence is a
    // whole slice, so the code below is the single-sequence step on offset pointers: no byte of another sequence is read or written.
    const size_t seq = blockIdx.z;
    qkv += seq * (size_t)(n_q + 2 * n_kv) * DA_HD;
    cosv += seq * DA_HD;
    sinv += seq * DA_HD;
    kc += seq * (size_t)n_kv * max_len * DA_HD;
    vc += seq * (size_t)n_kv * max_len * DA_HD;
    ws += seq * (size_t)n_q * nchunk * DA_PART;
    const int G = n_q / n_kv, p = (int)min(max(pos_p[seq], 0ll), (long long)max_len - 1), half = DA_HD / 2;   // (a position outside the cache is clamped, never written past it)
    float* out = ws + ((size_t)(kvh * nchunk + c) * G) * DA_PART;
    const int j0 = c * DA_CH, nkeys = min(DA_CH, p + 1 - j0);
    const bool owner = p >= j0 && p < j0 + DA_CH;
    if (nkeys > 0) {
        // ---- the chunk's rows: all requests of a thread in flight at once (rows past the prefix re-read its last row: finite, masked below)
        u32x4 kr[DA_PIECES], vr[DA_PIECES];
#pragma unroll
        for (int i = 0; i < DA_PIECES; ++i) {
            const int pc = tid + 256 * i, row = min(pc >> 4, nkeys - 1), col = pc & 15;
            const size_t off = ((size_t)kvh * max_len + j0 + row) * DA_HD + col * 8;
            kr[i] = *(const u32x4*)(kc + off);
            vr[i] = *(const u32x4*)(vc + off);
        }
        auto rope = [&](const T* src, int i) { return da_rope(src, cosv, sinv, half, i); };
        for (int i = tid; i < G * DA_HD; i += 256) qs[i / DA_HD][i % DA_HD] = rope(qkv + (size_t)(kvh * G + i / DA_HD) * DA_HD, i % DA_HD);
#pragma unroll
        for (int i = 0; i < DA_PIECES; ++i) {
            const int pc = tid + 256 * i;
            *(u32x4*)(ks + (pc >> 4) * DA_ROW + (pc & 15) * 16) = kr[i];
            *(u32x4*)(vs + (pc >> 4) * DA_ROW + (pc & 15) * 16) = vr[i];
        }
        __syncthreads();
        if (owner && tid < DA_HD) {   // the new token's key (rotated) and value: into the cache AND over the (stale) row of the LDS image
            const T kn = (T)rope(qkv + (size_t)(n_q + kvh) * DA_HD, tid), vn = qkv[(size_t)(n_q + n_kv + kvh) * DA_HD + tid];
            kc[((size_t)kvh * max_len + p) * DA_HD + tid] = kn;
            vc[((size_t)kvh * max_len + p) * DA_HD + tid] = vn;
            ((T*)(ks + (p - j0) * DA_ROW))[tid] = kn;
            ((T*)(vs + (p - j0) * DA_ROW))[tid] = vn;
        }
        __syncthreads();
        // ---- scores: a wave takes four keys per step, 16 lanes x 16 bytes per key row
        const int sub = lane >> 4, l16 = lane & 15;
        for (int jj = wv * (DA_CH / 4); jj < (wv + 1) * (DA_CH / 4); jj += 4) {
            const int j = jj + sub;
            float kf[8];
            unpack8<T>(*(const u32x4*)(ks + j * DA_ROW + l16 * 16), kf);
            for (int g = 0; g < G; ++g) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = __builtin_fmaf(kf[e], qs[g][l16 * 8 + e], d);
                d = da_row16_sum(d);
                if (l16 == 0) sc[g][j] = j < nkeys ? (float)(T)d * scale : -INFINITY;    // (the unfused path holds the scores in T)
            }
        }
        __syncthreads();
        for (int g = wv; g < G; g += 4) {          // chunk maximum, exponentials, sum: one wave per head
            constexpr int PER = DA_CH / 64;
            float v[PER], m = -INFINITY;
#pragma unroll
            for (int i = 0; i < PER; ++i) { v[i] = sc[g][lane + 64 * i]; m = fmaxf(m, v[i]); }
            m = wave_max(m);
            float l = 0.f;
#pragma unroll
            for (int i = 0; i < PER; ++i) { v[i] = __expf(v[i] - m); l += v[i]; sc[g][lane + 64 * i] = v[i]; }
            l = wave_sum(l);
            if (lane == 0) { ml[g][0] = m; ml[g][1] = l; }
        }
        __syncthreads();
        // ---- P V: wave = head (groups of four); four value rows per LDS instruction, each lane its eight channels over the keys of its quarter
        for (int g = wv; g < G; g += 4) {
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            for (int jb = 0; jb < nkeys; jb += 4) {
                const int j = jb + sub;
                float vf[8];
                unpack8<T>(*(const u32x4*)(vs + j * DA_ROW + l16 * 16), vf);     // (rows past nkeys: copies of the last row, weight exp(-inf) = 0)
                const float pw = sc[g][j];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(pw, vf[e], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[e] += __shfl_xor(acc[e], 16);
                acc[e] += __shfl_xor(acc[e], 32);
            }
            float* o = out + (size_t)g * DA_PART;
            if (sub == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[l16 * 8 + e] = acc[e];
            }
            if (lane == 0) { o[DA_HD] = ml[g][0]; o[DA_HD + 1] = ml[g][1]; }
        }
    } else {                                   // nothing of this chunk is visible yet
        for (int i = tid; i < G * DA_PART; i += 256) out[i] = (i % DA_PART) == DA_HD ? -INFINITY : 0.f;
    }
}

// folds the chunks of one query head: out = sum_c exp(m_c - M) acc_c / sum_c exp(m_c - M) l_c.  (A second launch, not a "last workgroup"
// ticket inside da_kernel: the partials of one head are written on several XCDs, and making them visible to one another inside a launch
// costs every workgroup an L2 write-back -- measured 41 us per call against 21 + 13 for two launches.)  The chunk loop is unrolled so that
// its loads are in flight together: one L2 latency, not one per chunk.
template <typename T>
__global__ __launch_bounds__(DA_HD) void da_combine_kernel(const float* __restrict__ ws, T* __restrict__ out, int n_q, int n_kv, int nchunk) {
    __shared__ float wsh[64];
    const int h = blockIdx.x, G = n_q / n_kv, kvh = h / G, g = h % G, d = threadIdx.x;
    ws += (size_t)blockIdx.y * n_q * nchunk * DA_PART;     // blockIdx.y: the sequence, as in da_kernel
    out += (size_t)blockIdx.y * n_q * DA_HD;
    const float* base = ws + ((size_t)kvh * nchunk * G + g) * DA_PART;
    const size_t cs = (size_t)G * DA_PART;
    float l = 0.f, acc = 0.f;
    for (int c0 = 0; c0 < nchunk; c0 += 64) {              // (<= 64 chunks per round: 8 192 keys)
        const int nc = min(64, nchunk - c0);
        float mc = -INFINITY, lc = 0.f;
        if (d < nc) { mc = base[(c0 + d) * cs + DA_HD]; lc = base[(c0 + d) * cs + DA_HD + 1]; }
        // running maximum across rounds is not needed for <= 64 chunks; for more, rescale
        const float Mr = wave_max(d < 64 ? mc : -INFINITY);
        __shared__ float Msh, Lsh, Ash;
        if (d == 0) { Msh = Mr; }
        __syncthreads();
        const float wgt = (d < nc && mc != -INFINITY) ? __expf(mc - Msh) : 0.f;
        if (d < 64) wsh[d] = wgt;
        const float lsum = wave_sum(d < 64 ? wgt * lc : 0.f);
        if (d == 0) Lsh = lsum;
        __syncthreads();
        float a = 0.f;
#pragma unroll 8
        for (int c = 0; c < nc; ++c) a = __builtin_fmaf(wsh[c], base[(c0 + c) * cs + d], a);
        if (c0 == 0) { acc = a; l = Lsh; Ash = Msh; }
        else {   // a later round: bring both to the larger maximum
            const float Mo = Ash, Mn = fmaxf(Mo, Msh), so = __expf(Mo - Mn), sn = __expf(Msh - Mn);
            acc = acc * so + a * sn; l = l * so + Lsh * sn;
            __syncthreads();
            if (d == 0) Ash = Mn;
        }
        __syncthreads();
    }
    out[(size_t)h * DA_HD + d] = (T)(acc / l);
}

// ==== the MFMA form
using rsvld_plan::DAM_RANGE;
constexpr int DAM_PSTRIDE = DA_PART + 2;   // floats between the partials of two heads in LDS: 16-byte aligned rows
static_assert(4 * A128_TILE == rsvld_plan::DAM_LDS_BYTES && 4 * DA_GMAX * DAM_PSTRIDE * 4 <= 2 * A128_TILE, "the waves' partials fit over the K tiles");

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
    __shared__ __attribute__((aligned(16))) char smem[4 * A128_TILE];   // K[2] | V[2]; after the products the waves' partials over K
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

    // ---- both tiles, requested at once (attention_d128.h; K[2] | V[2]); rows above p re-read row p (< max_len, written by the prologue).
    // A tile wholly above p is not requested (and not read: its waves are off).
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k0 = j0 + t * 64;
        if (k0 > p) break;
        const uint32_t kd = lds0 + t * A128_TILE + wu * 4096, vd = kd + 2 * A128_TILE;
        if (k0 + 63 <= p) {
            const char* kb = (const char*)(Kb + (size_t)(k0 + wu * 16) * D);
            const char* vb = (const char*)(Vb + (size_t)(k0 + wu * 16) * D);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * i + (lane >> 4);
                rsvld_lds_dma16(kb, (uint32_t)(rr * 256) + (uint32_t)a128_k_swz(lane, rr), kd + i * 1024);
                rsvld_lds_dma16(vb, (uint32_t)(rr * 256) + (uint32_t)a128_v_swz(lane, rr), vd + i * 1024);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * i + (lane >> 4);
                const int key = min(k0 + wu * 16 + rr, p);
                rsvld_lds_dma16_addr((const char*)(Kb + (size_t)key * D) + a128_k_swz(lane, rr), kd + i * 1024);
                rsvld_lds_dma16_addr((const char*)(Vb + (size_t)key * D) + a128_v_swz(lane, rr), vd + i * 1024);
            }
        }
    }

    // ---- Q fragments (B operand: col = the head on the lane, k = d); a padding column repeats the group's last head
    const int hq = kvh * G + min(l31, G - 1);
    const T* Qr = qrot + (seq * n_q + hq) * D;
    v8 qf[8];
    a128_load_q<T>(Qr, lh, qf);
    a128_pin_q(qf);
    __syncthreads();   // the tiles landed

    // wave w: keys kw0 .. kw0 + 31 = rows 32 (w & 1) .. of tile w >> 1
    const int kw0 = j0 + 32 * w;
    const bool wave_on = kw0 <= p;                                     // (wave-uniform)
    f32x16 oacc[4];
    float m_w = -INFINITY, l_w = 0.f;
    if (wave_on) {
        const int tile = w >> 1, kt = w & 1;
        const char* Ks = smem + tile * A128_TILE + kt * 8192;
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const v8 kf = *(const v8*)(Ks + a128_k_off(l31, lh, ks));
            sacc = Mfma<T>::mma(kf, qf[ks], sacc);
        }
        // ---- scale in fp32; the keys above p by selection (a NaN score of such a key never enters the arithmetic)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] *= scale;
        const bool edge = kw0 + 31 > p;                                // (wave-uniform)
        if (edge) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kw0 + a128_key(r, lh) > p) sacc[r] = -INFINITY;
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
        // ---- O^T[d][head] = V^T P^T: the wave's two 16-key groups 2 kt + s of its V tile (attention_d128.h: the transposed read)
        const int qq = (lane >> 2) & 3, pp = lane & 3, g1 = (lane >> 4) & 1;
        const int vbase = 2 * A128_TILE + tile * A128_TILE + (4 * lh + qq) * 256 + ((2 * g1 + (pp >> 1)) << 4) + ((pp & 1) << 3);
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
                if (edge) {   // keys above p: zero V registers (0 x NaN would be NaN)
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

// ---- host side: the checks both forms make first, the combine both launch last
int da_check(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, const void* kcache, const void* vcache, const void* out,
             const float* ws, int n_q, int n_kv, int max_len, int B, int dtype) {
    if (!qkv || !cosv || !sinv || !pos || !kcache || !vcache || !out || !ws) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (n_q <= 0 || n_kv <= 0 || max_len <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return RSVLD_EINVAL;
    return RSVLD_OK;
}

// partials [B][n_q x nchunk x DA_PART] -> out [B][n_q x 128]
template <typename T>
void da_combine_launch(const float* part, void* out, int n_q, int n_kv, int nchunk, int B, hipStream_t s) {
    hipLaunchKernelGGL((da_combine_kernel<T>), dim3(n_q, B), dim3(DA_HD), 0, s, part, (T*)out, n_q, n_kv, nchunk);
}

template <typename T>
void da_launch(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache, void* vcache, void* out, float* ws,
               int n_q, int n_kv, int max_len, int B, float scale, hipStream_t s) {
    const int nchunk = (max_len + DA_CH - 1) / DA_CH;
    hipLaunchKernelGGL((da_kernel<T>), dim3(n_kv, nchunk, B), dim3(256), 0, s, (const T*)qkv, (const T*)cosv, (const T*)sinv,
                       (const long long*)pos, (T*)kcache, (T*)vcache, ws, n_q, n_kv, max_len, scale);
    da_combine_launch<T>(ws, out, n_q, n_kv, nchunk, B, s);
}

// floats of the MFMA form's workspace: [B][n_q][128] rotated q in T (two to a float), then -- from *part on -- the partials
size_t dam_ws_floats(int n_q, size_t ranges, int B, size_t* part) {
    *part = (size_t)B * n_q * (DA_HD / 2);
    return *part + (size_t)B * n_q * ranges * DA_PART;
}

template <typename T>
void dam_launch(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache, void* vcache, void* out, float* ws,
                int n_q, int n_kv, int max_len, int B, float scale, int ranges, hipStream_t s) {
    size_t part_at;
    dam_ws_floats(n_q, ranges, B, &part_at);
    T* qrot = (T*)ws;
    float* part = ws + part_at;
    hipLaunchKernelGGL((dam_prologue_kernel<T>), dim3(n_q + n_kv, B), dim3(DA_HD), 0, s, (const T*)qkv, (const T*)cosv, (const T*)sinv,
                       (const long long*)pos, (T*)kcache, (T*)vcache, qrot, n_q, n_kv, max_len);
    hipLaunchKernelGGL((dam_kernel<T>), dim3(n_kv, ranges, B), dim3(256), 0, s, (const T*)qrot, (const long long*)pos, (const T*)kcache,
                       (const T*)vcache, part, n_q, n_kv, max_len, scale);
    da_combine_launch<T>(part, out, n_q, n_kv, ranges, B, s);
}

}  // namespace

// ---- the VALU form for B sequences (da_kernel takes the sequence from blockIdx.z); one sequence is the B = 1 call
extern "C" size_t rsvld_llama_decode_attention_rows_ws_bytes(int n_q, int n_kv, int max_len, int B) {
    if (n_q <= 0 || n_kv <= 0 || max_len <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return 0;
    return (size_t)B * n_q * ((max_len + DA_CH - 1) / DA_CH) * DA_PART * sizeof(float);
}

extern "C" size_t rsvld_llama_decode_attention_ws_bytes(int n_q, int n_kv, int max_len) {
    return rsvld_llama_decode_attention_rows_ws_bytes(n_q, n_kv, max_len, 1);
}

extern "C" int rsvld_llama_decode_attention_rows(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache, void* vcache,
                                                 void* out, float* ws, int n_q, int n_kv, int head_dim, int max_len, int B, float scale, int dtype,
                                                 void* stream) {
    if (const int rc = da_check(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, dtype); rc != RSVLD_OK) return rc;
    if (head_dim != DA_HD || n_q % n_kv != 0 || n_q / n_kv > DA_GMAX) return RSVLD_EUNSUPPORTED;
    if (((uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)qkv) & 15) return RSVLD_EINVAL;
    (dtype == RSVLD_F16 ? da_launch<f16> : da_launch<bf16>)(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, scale,
                                                            (hipStream_t)stream);
    return rsvld_check_launch();
}

extern "C" int rsvld_llama_decode_attention(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache, void* vcache,
                                            void* out, float* ws, int n_q, int n_kv, int head_dim, int max_len, float scale, int dtype,
                                            void* stream) {
    return rsvld_llama_decode_attention_rows(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, head_dim, max_len, 1, scale, dtype, stream);
}

// ---- the MFMA form
extern "C" int rsvld_plan_llama_decode_attention_mma(int n_q, int n_kv, int max_len, int dtype, rsvld_decode_attention_mma_plan* plan) {
    if (plan == nullptr) return RSVLD_EINVAL;
    return rsvld_plan::plan_decode_attention_mma(n_q, n_kv, max_len, dtype, plan);
}

extern "C" size_t rsvld_llama_decode_attention_mma_rows_ws_bytes(int n_q, int n_kv, int max_len, int B) {
    if (n_q <= 0 || n_kv <= 0 || max_len <= 0 || B < 1 || B > RSVLD_DECODE_MAX_ROWS) return 0;
    size_t part_at;
    return dam_ws_floats(n_q, ((size_t)max_len + DAM_RANGE - 1) / DAM_RANGE, B, &part_at) * sizeof(float);
}

extern "C" int rsvld_llama_decode_attention_mma_rows(const void* qkv, const void* cosv, const void* sinv, const int64_t* pos, void* kcache,
                                                     void* vcache, void* out, float* ws, int n_q, int n_kv, int head_dim, int max_len, int B,
                                                     float scale, int dtype, void* stream) {
    if (const int rc = da_check(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, dtype); rc != RSVLD_OK) return rc;
    if (head_dim != DA_HD) return RSVLD_EUNSUPPORTED;
    rsvld_decode_attention_mma_plan pl;
    const int rc = rsvld_plan::plan_decode_attention_mma(n_q, n_kv, max_len, dtype, &pl);
    if (rc != RSVLD_OK) return rc;
    if (((uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)qkv | (uintptr_t)ws) & 15) return RSVLD_EINVAL;
    (dtype == RSVLD_F16 ? dam_launch<f16> : dam_launch<bf16>)(qkv, cosv, sinv, pos, kcache, vcache, out, ws, n_q, n_kv, max_len, B, scale,
                                                              pl.ranges, (hipStream_t)stream);
    return rsvld_check_launch();
}
