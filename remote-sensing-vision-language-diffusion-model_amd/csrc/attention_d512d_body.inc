// Included by attention_d512d.inc THREE times inside attn_d512d_kernel: the body of the key-tile loop (iteration t).
// A5_STEADY = 1: tiles t .. t + 3 exist and are full (no bound tests, no ragged mask); A5_PAIR = 1: the two score register
// sets S_CUR / S_NXT swap roles between the two bodies of a trip.  A5_STEADY = A5_PAIR = 0: the general body (last tiles).
        const bool more = A5_STEADY ? true : t + 1 < nt;
        const int b_pv = t & 3, pb = (t & 1) * A5D_PBUF, ab = (t & 1) * 512;

        // ---- phase A: S(t+1) beside the online softmax of tile t (attention_d512_softmax.inc, in 7 hook parts)
        float mx = -INFINITY, alpha = 1.0f, rs = 0.f;
        bool need = false;
        v8 pf[2];
        auto sm = [&](int part) {
#include "attention_d512_softmax.inc"
        };
#if !A5_PAIR
        f32x16 snext;
#endif
        if (more) {
#define A5D_HOOK(i) \
    sm(i);          \
    __builtin_amdgcn_sched_barrier(0)
            if constexpr (__is_same(T, f16)) {
                A5_CHAIN("v_mfma_f32_32x32x16_f16", S_NXT, ((t + 1) & 3), A5D_HOOK);
            } else {
                A5_CHAIN("v_mfma_f32_32x32x16_bf16", S_NXT, ((t + 1) & 3), A5D_HOOK);
            }
#undef A5D_HOOK
        } else {
#pragma unroll
            for (int i = 0; i < 7; ++i) sm(i);
        }

        // publish P(t) (lane for lane: another wave's B operand of this q-block has this lane layout) and alpha(t)
        *(v8*)(smem + pb + p_own) = pf[0];
        *(v8*)(smem + pb + p_own + 1024) = pf[1];
        *(float*)(smem + ab + a_own) = alpha;   // (both half-waves store the same value)
        // X^T(t) fragments of this wave's d-slice: A operand of k-step s2, elements 0..3 = keys 16s2 + 4lh + 0..3, 4..7 = +8
        v8 vfr[2][4];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int f = 0; f < 4; ++f) vfr[s2][f] = vread(b_pv, f, s2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of tile t+2 have landed
        __syncthreads();   // P(t) / alpha(t) of every wave written; X(t+2) complete; PV(t-1) done with ring buffer (t+3) & 3

        // ---- phase B: O^T[d-slice][all 128 rows] += X^T P^T
        v8 pfo[2][3];
        float al[3];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 3; ++j) pfo[s2][j] = *(const v8*)(smem + pb + p_oth[j] + 1024 * s2);
#pragma unroll
        for (int j = 0; j < 3; ++j) al[j] = *(const float*)(smem + ab + a_oth[j]);

        // O lives in the accumulator file: acc_scale
        if (__builtin_expect(__any(need), 0)) {   // own rows (cold)
            asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) acc_scale(oacc[dt][0], alpha);
        }
        __builtin_amdgcn_sched_barrier(0);
        // own q-block first: its P is in registers, the other blocks' P is still on its way from LDS
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                oacc[f][0] = Mfma<T>::mma(vfr[s2][f], pf[s2], oacc[f][0]);
                __builtin_amdgcn_sched_barrier(0);
            }
        // the other q-blocks' rescale: alpha is exactly 1 on every row whose max did not move, so scaling a whole block
        // whenever any of its rows moved gives what the row's own wave would have done
        if (__builtin_expect(__any(al[0] != 1.0f || al[1] != 1.0f || al[2] != 1.0f), 0)) {
            asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) acc_scale(oacc[dt][j + 1], al[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
        // 24 MFMAs; the 8 LDS-DMA rows of tile t+3 behind every third
#pragma unroll
        for (int n = 0; n < 24; ++n) {
            const int s2 = n / 12, f = (n / 3) & 3, j = n % 3;
            oacc[f][j + 1] = Mfma<T>::mma(vfr[s2][f], pfo[s2][j], oacc[f][j + 1]);
            if (n % 3 == 2) {
                if (A5_STEADY) {
                    dma_x_fast(t + 3, n / 3);
                } else if (t + 3 < nt) {
                    dma_x(t + 3, n / 3);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#if !A5_PAIR
        if (more) S_CUR = S_NXT;   // readable by VALU: 32 PV MFMAs have issued since the chain's last MFMA
#endif
