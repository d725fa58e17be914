// Included by attention_d512d.inc THREE times inside attn_d512d_kernel: the body of the key-tile loop (iteration t).
// A5D_STEADY = 1: tiles t .. t + 3 exist and are full (no bound tests, no ragged mask); A5D_PAIR = 1: the two score register
// sets S_CUR / S_NXT swap roles between the two bodies of a trip.  A5D_STEADY = A5D_PAIR = 0: the general body (last tiles).
        const bool more = A5D_STEADY ? true : t + 1 < nt;
        const int b_pv = t & 3, pb = (t & 1) * A5D_PBUF, ab = (t & 1) * 512;

        // ---- phase A: S(t+1) beside the online softmax of tile t (the softmax of attention_d512_body.inc, in 7 hook parts)
        float mx = -INFINITY, alpha = 1.0f, rs = 0.f;
        bool need = false;
        v8 pf[2];
        auto sm = [&](int part) {
            if (part == 0) {
                if (!A5D_STEADY && k_begin + (t + 1) * 32 > k_end) {   // ragged last tile (uniform branch)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kv = k_begin + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (kv >= k_end) S_CUR[r] = -INFINITY;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S_CUR[r]);
                asm volatile("" : "+v"(S_CUR), "+v"(mx));
            } else if (part == 1) {
                mx = a5b_halfwave_max(mx) * p.scale_log2e;
                need = mx > m_run + A5_DEFER_LOG2;   // deferred max; true on the first tile (m_run = -inf)
                if (need) {
                    alpha = __builtin_amdgcn_exp2f(m_run - mx);
                    m_run = mx;
                }
                asm volatile("" : "+v"(alpha), "+v"(m_run));
            } else if (part >= 2 && part <= 5) {
                const int r0 = 4 * (part - 2);
#pragma unroll
                for (int r = r0; r < r0 + 4; ++r) {
                    S_CUR[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(S_CUR[r], p.scale_log2e, -m_run));
                    rs += S_CUR[r];
                }
                asm volatile("" : "+v"(S_CUR[r0]), "+v"(S_CUR[r0 + 1]), "+v"(S_CUR[r0 + 2]), "+v"(S_CUR[r0 + 3]), "+v"(rs));
            } else if (part == 6) {
                l_run = l_run * alpha + rs;
                // P as the B operand of k-step s: registers 8s..8s+7 <-> keys 16s + 8(j>>2) + 4lh + (j&3)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[s2][j] = (T)S_CUR[8 * s2 + j];
                asm volatile("" : "+v"(pf[0]), "+v"(pf[1]), "+v"(l_run));
            }
        };
#if !A5D_PAIR
        f32x16 snext;
#endif
        if (more) {
#define A5D_HOOK(i) \
    sm(i);          \
    __builtin_amdgcn_sched_barrier(0)
            if constexpr (__is_same(T, f16)) {
                A5D_CHAIN("v_mfma_f32_32x32x16_f16", S_NXT, ((t + 1) & 3), A5D_HOOK);
            } else {
                A5D_CHAIN("v_mfma_f32_32x32x16_bf16", S_NXT, ((t + 1) & 3), A5D_HOOK);
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

        // O lives in the accumulator file: rescaled one element at a time through a scratch VGPR (see attention_d512_body.inc)
#define A5D_RESCALE(J, A)                                                                                                  \
    _Pragma("unroll") for (int dt = 0; dt < 4; ++dt)                                                                       \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                       \
        float x = oacc[dt][J][r], tmp;                                                                                     \
        asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\ts_nop 0\n\tv_accvgpr_write_b32 %0, %1\n\ts_nop 1" \
                     : "+a"(x), "=&v"(tmp)                                                                                 \
                     : "v"(A));                                                                                            \
        oacc[dt][J][r] = x;                                                                                                \
    }
        if (__builtin_expect(__any(need), 0)) {   // own rows (cold)
            asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
            A5D_RESCALE(0, alpha)
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
            A5D_RESCALE(1, al[0])
            A5D_RESCALE(2, al[1])
            A5D_RESCALE(3, al[2])
        }
#undef A5D_RESCALE
        __builtin_amdgcn_sched_barrier(0);
        // 24 MFMAs; the 8 LDS-DMA rows of tile t+3 behind every third
#pragma unroll
        for (int n = 0; n < 24; ++n) {
            const int s2 = n / 12, f = (n / 3) & 3, j = n % 3;
            oacc[f][j + 1] = Mfma<T>::mma(vfr[s2][f], pfo[s2][j], oacc[f][j + 1]);
            if (n % 3 == 2) {
                if (A5D_STEADY) {
                    dma_x_fast(t + 3, n / 3);
                } else if (t + 3 < nt) {
                    dma_x(t + 3, n / 3);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#if !A5D_PAIR
        if (more) S_CUR = S_NXT;   // readable by VALU: 32 PV MFMAs have issued since the chain's last MFMA
#endif
