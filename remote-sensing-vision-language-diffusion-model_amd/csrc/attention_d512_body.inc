// Included by attention.hip THREE times inside attn_d512b_kernel: the body of the key-tile loop.  A5_STEADY = 1: tiles t + 1 and
// t + 2 exist and are full (branch-free around the chain and the requests); A5_PAIR = 1: the steady-state loop runs two bodies per
// trip with the two score register sets S_CUR / S_NXT swapped, so that no S_CUR <- S_NXT copy exists (16 moves per tile -- which
// hipcc, knowing no latency for the result of an asm MFMA, placed three instructions behind the chain's last MFMA in a branch-free
// body: stale scores, errors of 1e-3 .. 1e-1 in the shared-tile tests).  A5_STEADY = A5_PAIR = 0: the general body (last tiles).
        // A5_STEADY (set by the including file): t + 3 < nt, i.e. tiles t + 1 and t + 2 exist and are FULL -- no branch around the S
        // chain, the LDS-DMA requests or the ragged-tile mask (one wave per SIMD: nobody covers a branch's instruction-fetch bubble)
        const bool more = A5_STEADY ? true : t + 1 < nt, more2 = A5_STEADY ? true : t + 2 < nt;
        const int b_s = b_pv == 2 ? 0 : b_pv + 1, b_dma = b_pv == 0 ? 2 : b_pv - 1;   // (t + 1) % 3, (t + 2) % 3
        const int vb = (SH ? b_pv : (t & 1)) * A5B_TILE;

        // ---- online softmax of tile t (attention_d512_softmax.inc) in the hooks of the S(t+1) chain
        float mx = -INFINITY, alpha = 1.0f, rs = 0.f;
        bool need = false;
        v8 pf[2];
        auto sm = [&](int part) {
            if (A5B_ABL & 1) {
                if (part == 6) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int j = 0; j < 8; ++j) pf[s2][j] = (T)S_CUR[8 * s2 + j];
                    asm volatile("" : "+v"(pf[0]), "+v"(pf[1]), "+v"(l_run));
                }
                return;
            }
#include "attention_d512_softmax.inc"
        };

#if !A5_PAIR
        f32x16 snext;
#endif
        if (more) {
#define A5B_HOOK(i)                                                   \
    if constexpr (SH) {                                               \
        if (more2) dma_kb_s(t + 2, b_dma, i);                           \
    } else {                                                          \
        if (more2) dma_k_s(t + 2, i);                                   \
        dma_v_s(t + 1, i);                                            \
    }                                                                 \
    sm(i);                                                            \
    __builtin_amdgcn_sched_barrier(0)
            if constexpr (__is_same(T, f16)) {
                A5_CHAIN("v_mfma_f32_32x32x16_f16", S_NXT, (SH ? b_s : ((t + 1) & 1)), A5B_HOOK);
            } else {
                A5_CHAIN("v_mfma_f32_32x32x16_bf16", S_NXT, (SH ? b_s : ((t + 1) & 1)), A5B_HOOK);
            }
#undef A5B_HOOK
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) sm(i);
        }

        // first V fragments of PV(t)
        constexpr int VD = 5;
        auto vread = [&](int n) {
            const int dt = n >> 1, s2 = n & 1;
            const int off = vb + vbase[dt & 3] + (dt >> 2) * 256 + (16 * s2) * 1024;
            // rows +8 (hf = 1): in the shared image the low swizzle bits are (lh + 2 hf) & 3, i.e. chunk bit 1 flips
            return tr16_pair<v8>(lds_read_tr16(smem + off), lds_read_tr16(smem + ((SH ? (off ^ 32) : off) + 8 * 1024)));
        };
        v8 vfr[VD];
#pragma unroll
        for (int i = 0; i < VD; ++i) vfr[i] = vread(i);

        if (__builtin_expect(__any(need), 0)) {   // (cold: the rescale block is laid out behind the loop)
            // O lives in the accumulator file: acc_scale (written as plain C++ hipcc spills 375 registers here).  The MFMA -> read
            // hazard is covered by the 32 S-chain MFMAs (or the epilogue of the previous PV) before this point.
            asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
#pragma unroll
            for (int dt = 0; dt < 16; ++dt) acc_scale(oacc[dt], alpha);
        }

        // ---- O^T[d][q] += V^T P^T; the A operand (row = d, k = the same key order) is two transposed reads:
        // elements 0..3 = keys 16s + 4lh + 0..3, elements 4..7 = keys 16s + 8 + 4lh + 0..3.  Explicit fragment ring.
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 32; ++n) {
            oacc[n >> 1] = Mfma<T>::mma(vfr[n % VD], pf[n & 1], oacc[n >> 1]);
            if (n + VD < 32 && !(A5B_ABL & 2)) vfr[n % VD] = vread(n + VD);
            __builtin_amdgcn_sched_barrier(0);
        }
#if !A5_PAIR
        if (more) S_CUR = S_NXT;   // readable by VALU: 32 PV MFMAs have issued since the chain's last MFMA
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of the next tiles have landed
        if (!(A5B_ABL & 16)) __syncthreads();   // everyone done with this tile's buffers (ablation 16: no barrier -- results WRONG, timing only)
        b_pv = b_s;
