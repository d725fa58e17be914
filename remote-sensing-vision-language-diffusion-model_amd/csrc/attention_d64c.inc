// Included by attention.hip inside its anonymous namespace (uses AttnArgs, Mfma<T>, A6B_TILE, a6b_add).
// ---------------------------------------------------------------------------------------
// D = 64, the "ping-pong" form.  attn_d64b runs four waves per SIMD whose phases are left to chance: the
// matrix pipe is busy 61 % of the time (PMC) although the kernel's vector issue (exp 8, add 4, cvt 4 cycles per instruction;
// MI355X_MICROARCH.md) would allow ~0.9.  Here the overlap is by construction:
//   * one workgroup of 8 waves per CU (two per SIMD, up to 256 registers); a wave owns 64 query rows (two 32-row sub-tiles
//     j = 0, 1 that share every K / V fragment read), the workgroup 512;
//   * every wave's loop body is two SEGMENTS per 64-key tile:
//        M (matrix):  PV of tile i (16 MFMAs), then the S chains of tile i + 1 (20 MFMAs incl. the bias steps), with the
//                     K-fragment reads of tile i + 1 and the LDS-DMA request of tile i + 3 in the first gaps: no vector work;
//        V (vector):  the sum-checked softmax of a tile (exp2, row sums, 16-bit P) and the V-fragment reads for the next M;
//     waves 0..3 run M then V, waves 4..7 (the second wave of every SIMD) V then M, so on every SIMD a matrix segment runs
//     beside a vector segment (cdna_hip_programming.md T5 / MI355X_MICROARCH.md "Two waves per SIMD"); ONE raw s_barrier per tile;
//   * K / V tiles in a 4-deep LDS-DMA ring: tile i + 3 is requested in period i and first read in period i + 2 (S) / i + 3
//     (PV, redo); its landing is waited for with a counted vmcnt at the end of period i + 1; the buffer it overwrites held tile
//     i - 1, last read in period i - 1;
//   * arithmetic IDENTICAL to attn_d64b (same MFMA chains, same exp2 / row-sum order, same sum check and redo), so the two
//     kernels agree bit for bit and the choice between them (A6C_MIN_WG, rsvld_plan.h) is not a numerics decision.
// ---------------------------------------------------------------------------------------
#ifndef A6C_ABL
#define A6C_ABL 0   // diagnostic builds (results WRONG, timing only): 1 no in-loop LDS-DMA request, 2 no exponentials, 4 no row sums,
                    // 8 no softmax at all (V segment = V reads only), 16 no MFMAs in the M segment
#endif
// MODE 0: C = 0 (first step of a chain, behind a VALU write), 1: accumulate, 2: accumulate behind a VALU write
template <typename T, int MODE>
__device__ __forceinline__ void a6c_mma(f32x16& acc, const typename Mfma<T>::v8& a, const typename Mfma<T>::v8& b) {
    if constexpr (__is_same(T, f16)) {
        if constexpr (MODE == 0) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
        else if constexpr (MODE == 2) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
    } else {
        if constexpr (MODE == 0) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
        else if constexpr (MODE == 2) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
    }
}

constexpr int A6C_SMEM = 2 * 4 * A6B_TILE + 8 * A6B_TILE;   // ring + Q image = 128 KiB
template <typename T>
__global__ __launch_bounds__(512, 2) void attn_d64c_kernel(AttnArgs p) {
    constexpr int D = 64, NB = 4;
    typedef typename Mfma<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // K[4] | V[4] | Q (8 waves x 64 rows): A6C_SMEM bytes

    const int tid = threadIdx.x, lane = tid & 63;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wu = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool late = wu >= 4;   // the second wave of its SIMD
    // XCD-aware work order (rsvld_xcd_item) over (head, query block) items: with the plain (query block, head, batch) grid the 256
    // concurrent workgroups spread EVERY head over all 8 L2s (at 2 x 20 heads x 16 384 tokens: 8 heads x 4 MB of K / V per 4 MiB L2,
    // four CUs per stream); here an XCD's 32 CUs work on the same head's K / V stream in step.
    int qblk, h, b;
    {
        const int nqb = gridDim.x, nwg = gridDim.x * gridDim.y * gridDim.z;
        const int lid = blockIdx.x + nqb * (blockIdx.y + gridDim.y * blockIdx.z);
        const int t = rsvld_xcd_item(lid, nwg);
        qblk = t % nqb;
        const int bh = t / nqb;
        h = bh % gridDim.y;
        b = bh / gridDim.y;
    }
    const int q0 = (qblk * 8 + wu) * 64;
    const T* Qb = (const T*)p.q + (int64_t)b * p.q_bs + (int64_t)h * D;
    const T* Kb = (const T*)p.k + (int64_t)b * p.k_bs + (int64_t)h * D;
    const T* Vb = (const T*)p.v + (int64_t)b * p.v_bs + (int64_t)h * D;
    const int nt = (p.Nk + 63) >> 6;

    // ---- tile DMA (the LDS images and swizzles of attn_d64b): wave w moves key rows 8w .. 8w+7, one piece per tensor and tile
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
    const int64_t k_rowb = p.k_ts * (int64_t)sizeof(T), v_rowb = p.v_ts * (int64_t)sizeof(T);
    const int drow = lane >> 3, r16 = (wu * 8 + drow) & 15;
    const uint32_t kswz = (uint32_t)(((lane & 7) ^ ((r16 >> 1) & 7)) << 4), vswz = (uint32_t)(((lane & 7) ^ (((r16 >> 1) & 1) << 2)) << 4);
    const uint32_t kvo = (uint32_t)(drow * k_rowb) + kswz, vvo = (uint32_t)(drow * v_rowb) + vswz;
    // LDS-DMA pieces: rsvld_lds_dma16_m0, M0 declared clobbered instead of saved / restored: +1.1-1.2 % here, where attn_d64b lost 12 % with it
    const char* k_next = (const char*)(Kb + (int64_t)(wu * 8) * p.k_ts);   // requests come in tile order: two pointer adds each
    const char* v_next = (const char*)(Vb + (int64_t)(wu * 8) * p.v_ts);
    const int64_t k_step = 64 * k_rowb, v_step = 64 * v_rowb;
    auto dma_tile = [&](int t, bool known_full = false) __attribute__((always_inline)) {   // always exactly two pieces (the counted vmcnt below relies on it)
        const uint32_t kd = lds0 + (t & (NB - 1)) * A6B_TILE + wu * 1024, vd = kd + NB * A6B_TILE;
        if (known_full || t * 64 + 64 <= p.Nk) {
            rsvld_lds_dma16_m0(k_next, kvo, kd);
            rsvld_lds_dma16_m0(v_next, vvo, vd);
            k_next += k_step;
            v_next += v_step;
        } else {
            // ragged last tile: rows past Nk re-read the last key (their scores are masked).  Same instruction form: the scalar
            // base is the tile's FIRST row (the last tile holds at least one key), the clamped row goes into the lane offset
            const int rel = min(wu * 8 + drow, p.Nk - 1 - t * 64);   // >= 0
            rsvld_lds_dma16_m0((const char*)(Kb + (int64_t)(t * 64) * p.k_ts), (uint32_t)(rel * k_rowb) + kswz, kd);
            rsvld_lds_dma16_m0((const char*)(Vb + (int64_t)(t * 64) * p.v_ts), (uint32_t)(rel * v_rowb) + vswz, vd);
        }
    };
    dma_tile(0);
    if (nt > 1) dma_tile(1);
    if (nt > 2) dma_tile(2);

    // ---- Q, pre-scaled by scale * log2(e) (bias step, see attn_d64b), parked in LDS: every lane stores the eight fragments it
    // will need (B operand: col = query row on the lane, k = d) at the address it reads them back from in every S chain, in the
    // K-tile image (conflict-free ds_read_b128).  Held in registers the fragments cost 32 of the 256 for the whole kernel, and
    // hipcc spilled them to scratch around the early half's loop -- scratch reloads share vmcnt with the LDS-DMA prefetch.
    char* const Qs = smem + 2 * NB * A6B_TILE + wu * A6B_TILE;   // this wave's 64 rows x 128 B
    int koff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) koff[ks] = l31 * 128 + (((2 * ks + lh) ^ ((l31 >> 1) & 7)) << 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qrow = q0 + 32 * j + l31;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (qrow < p.Nq) v = *(const u32x4*)(Qb + (int64_t)qrow * p.q_ts + ks * 16 + lh * 8);
            v8 f = __builtin_bit_cast(v8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (T)((float)f[e] * p.scale_log2e);
            *(v8*)(Qs + j * 4096 + koff[ks]) = f;
        }
    }
    f32x16 oacc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[j][dt][r] = 0.f;
    float m_run[2] = {0.f, 0.f}, l_run[2] = {0.f, 0.f};
    uint32_t one_lo;   // A operand of the bias step, register 0: 1.0 in element 0 of lanes 0..31 (k-slot 0), zero elsewhere
    {
        T pair[2] = {lh == 0 ? (T)1.f : (T)0.f, (T)0.f};
        __builtin_memcpy(&one_lo, pair, 4);
    }
    int voff[2];
    {
        const int qq = (lane >> 2) & 3, pp = lane & 3, g1 = (lane >> 4) & 1;
        const int row = 4 * lh + qq;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            voff[dt] = NB * A6B_TILE + row * 128 + (((4 * dt + 2 * g1 + (pp >> 1)) ^ (((row >> 1) & 1) << 2)) << 4) + ((pp & 1) << 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // tiles 0..2 landed

    f32x16 sacc[2][2];   // [j][32-key half]
    v8 vf[2][4], pf[2][4];
    auto seg_barrier = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // operands of one k-step of the S chains: K fragments of both 32-key halves, Q fragments of both sub-tiles (16 registers)
    struct KStep { v8 k0, k1, q0, q1; };
    auto read_step = [&](int t, int ks) __attribute__((always_inline)) {
        const char* Ks = smem + (t & (NB - 1)) * A6B_TILE;
        KStep f;
        f.k0 = *(const v8*)(Ks + koff[ks]);
        f.k1 = *(const v8*)(Ks + 4096 + koff[ks]);
        f.q0 = *(const v8*)(Qs + koff[ks]);
        f.q1 = *(const v8*)(Qs + 4096 + koff[ks]);
        return f;
    };
    auto read_v = [&](int t) __attribute__((always_inline)) {
        const int vb = (t & (NB - 1)) * A6B_TILE;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int off = vb + voff[dt] + s4 * 2048;
                vf[dt][s4] = tr16_pair<v8>(lds_read_tr16(smem + off), lds_read_tr16(smem + off + 1024));
            }
    };
    // the three operand tuples of the bias steps live in 12 registers, zeros written once (rebuilt per tile: 10 v_mov_b32 in the matrix segment)
    u32x4 ones_t = {one_lo, 0u, 0u, 0u}, bias_t[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    asm volatile("" : "+v"(ones_t), "+v"(bias_t[0]), "+v"(bias_t[1]));
    auto bias_operands = [&](int j, v8& onesf, v8& biasf) __attribute__((always_inline)) {   // A = 1 in k-slot 0, B = -m of the lane's query there
        T pair[2] = {(T)(-m_run[j]), (T)0.f};
        uint32_t b0;
        __builtin_memcpy(&b0, pair, 4);
        bias_t[j][0] = b0;
        asm volatile("" : "+v"(ones_t), "+v"(bias_t[j]));   // the tuples stay where they are: no copies
        onesf = __builtin_bit_cast(v8, ones_t);
        biasf = __builtin_bit_cast(v8, bias_t[j]);
        (void)one_lo;   // keeps one_lo in this closure: without the capture hipcc swaps two score register ranges (same instructions, other register numbers)
    };
    auto mask_tail = [&](int t, int j) __attribute__((always_inline)) {
        if ((t + 1) * 64 > p.Nk) {   // ragged last tile only (uniform branch)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = t * 64 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (kv >= p.Nk) sacc[j][kt][r] = -INFINITY;
                }
        }
    };
    // S^T of tile t for BOTH query sub-tiles: four independent chains (j, half) of bias step + 4 k-steps, issued step-major so
    // that an MFMA never waits for the one before it; ``f0`` = the operands of k-step 0 (read by the caller, earlier), the
    // following steps' operands are read one step ahead
    auto s_chains = [&](int t, KStep f0, bool not_last = false) __attribute__((always_inline)) {
        v8 onesf, b0f, b1f;
        bias_operands(0, onesf, b0f);
        bias_operands(1, onesf, b1f);
        __builtin_amdgcn_sched_barrier(0);
        a6c_mma<T, 0>(sacc[0][0], onesf, b0f);
        a6c_mma<T, 0>(sacc[1][0], onesf, b1f);
        a6c_mma<T, 0>(sacc[0][1], onesf, b0f);
        a6c_mma<T, 0>(sacc[1][1], onesf, b1f);
        KStep f[4];
        f[0] = f0;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) f[ks + 1] = read_step(t, ks + 1);
            __builtin_amdgcn_sched_barrier(0);
            a6c_mma<T, 1>(sacc[0][0], f[ks].k0, f[ks].q0);
            a6c_mma<T, 1>(sacc[1][0], f[ks].k0, f[ks].q1);
            a6c_mma<T, 1>(sacc[0][1], f[ks].k1, f[ks].q0);
            a6c_mma<T, 1>(sacc[1][1], f[ks].k1, f[ks].q1);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sacc[0][0]), "+v"(sacc[0][1]), "+v"(sacc[1][0]), "+v"(sacc[1][1]));   // MFMA D -> VALU reader
        __builtin_amdgcn_sched_barrier(0);
        if (!not_last) {
            mask_tail(t, 0);
            mask_tail(t, 1);
        }
    };
    auto s_redo = [&](int t, int j) __attribute__((always_inline)) {   // the rare tile whose scores outgrew the bias: the scores of sub-tile j once more
        v8 onesf, bf;
        bias_operands(j, onesf, bf);
        a6c_mma<T, 0>(sacc[j][0], onesf, bf);
        a6c_mma<T, 0>(sacc[j][1], onesf, bf);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const KStep f = read_step(t, ks);
            a6c_mma<T, 1>(sacc[j][0], f.k0, j == 0 ? f.q0 : f.q1);
            a6c_mma<T, 1>(sacc[j][1], f.k1, j == 0 ? f.q0 : f.q1);
        }
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sacc[j][0]), "+v"(sacc[j][1]));
        mask_tail(t, j);
    };
    auto exp_and_sum = [&](int j) __attribute__((always_inline)) {   // P = exp2(s') in place -> the lane's row-sum share (four chains: latency, see attn_d64b)
        float r4[4];   // (chain g starts at its first exponential: 0 + x == x exactly, so this is attn_d64b's sum without four adds)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = (A6C_ABL & 2) ? sacc[j][kt][r] : __builtin_amdgcn_exp2f(sacc[j][kt][r]);
                sacc[j][kt][r] = pv;
                r4[r >> 2] = (kt == 0 && (r & 3) == 0) ? pv : ((A6C_ABL & 4) ? r4[r >> 2] : a6b_add(r4[r >> 2], pv));
            }
        return a6b_add(a6b_add(r4[0], r4[1]), a6b_add(r4[2], r4[3]));
    };
    // the rare tile whose row sum says the bias was stale (and the first tile): scores once more, exact maximum, rescale
    auto redo = [&](int t, int j, float& rs, float& alpha) __attribute__((always_inline)) {
        s_redo(t, j);
        float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) m4[r >> 2] = fmaxf(m4[r >> 2], sacc[j][kt][r]);
        float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        {
            const uint32_t mb = __builtin_bit_cast(uint32_t, mx);
            const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
            mx = fmaxf(__builtin_bit_cast(float, (uint32_t)sw[0]), __builtin_bit_cast(float, (uint32_t)sw[1]));
        }
        // both half-waves of a query take the same decision from the same mx: m_run stays equal in lane and lane ^ 32
        const bool up = (t == 0) || (mx > 0.0f);                        // the maximum only ever moves UP (alpha <= 1)
        const float m_new = up ? (float)(T)(m_run[j] + mx) : m_run[j];  // representable in T: next tile's bias operand
        const float delta = m_new - m_run[j];
        m_run[j] = m_new;
        alpha = t == 0 ? 1.0f : __builtin_amdgcn_exp2f(-delta);         // first tile: nothing to rescale (delta may be << 0)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[j][kt][r] -= delta;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[j][dt][r] *= alpha;
        rs = exp_and_sum(j);
    };
    auto to_p = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[j][s4][e] = (T)sacc[j][s4 >> 1][8 * (s4 & 1) + e];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) asm volatile("" : "+v"(pf[j][s4]));   // converted HERE (hipcc otherwise sinks the 32 cvt_pk into the next matrix segment)
    };
    // sum-checked softmax of tile t (see attn_d64b's loop), -> pf.  The exponentials and row sums of BOTH sub-tiles first, then ONE
    // wave-uniform branch for the rare redo (the decision per sub-tile is unchanged): one reduction tail + compare + scalar branch
    // per tile instead of two, in a segment with nobody to hide them behind.
    auto softmax = [&](int t) __attribute__((always_inline)) {
        float alpha0 = 1.0f, alpha1 = 1.0f;
        float rs0 = exp_and_sum(0), rs1 = exp_and_sum(1);
        const bool need0 = (t == 0) || !(rs0 <= 16384.0f), need1 = (t == 0) || !(rs1 <= 16384.0f);
        if (__builtin_expect(__any(need0 || need1), 0)) {   // (cold: laid out behind the loop, the hot path falls through)
            if (__any(need0)) redo(t, 0, rs0, alpha0);
            if (__any(need1)) redo(t, 1, rs1, alpha1);
        }
        l_run[0] = l_run[0] * alpha0 + rs0;
        l_run[1] = l_run[1] * alpha1 + rs1;
        to_p(0);
        to_p(1);
    };
    // O^T[d][q] += V^T P^T, one 16-key step for both sub-tiles and both d halves (four independent accumulators)
    auto pv_first = [&]() __attribute__((always_inline)) {
        a6c_mma<T, 2>(oacc[0][0], vf[0][0], pf[0][0]);
        a6c_mma<T, 2>(oacc[0][1], vf[1][0], pf[0][0]);
        a6c_mma<T, 2>(oacc[1][0], vf[0][0], pf[1][0]);
        a6c_mma<T, 2>(oacc[1][1], vf[1][0], pf[1][0]);
    };
    auto pv_step = [&](int s4) __attribute__((always_inline)) {
        a6c_mma<T, 1>(oacc[0][0], vf[0][s4], pf[0][s4]);
        a6c_mma<T, 1>(oacc[0][1], vf[1][s4], pf[0][s4]);
        a6c_mma<T, 1>(oacc[1][0], vf[0][s4], pf[1][s4]);
        a6c_mma<T, 1>(oacc[1][1], vf[1][s4], pf[1][s4]);
    };

    unsigned long long st_sum[4] = {0, 0, 0, 0}, st_t = 0;   // -DA6B_STAMP=1: M work | V work | vmcnt wait + barrier
#define A6C_MARK(i) do { if (A6B_STAMP) { const unsigned long long now_ = a6b_stamp(); st_sum[i] += now_ - st_t; st_t = now_; } } while (0)
    // M(i): PV(i), S(i + 1); the K fragments of tile i + 1 and the request of tile i + 3 go into the gaps behind the first MFMAs
    auto m_part = [&](int i, bool req, bool steady = false) __attribute__((always_inline)) {   // steady (a literal): tile i + 3 exists and is full, tile i + 1 is not the last
        asm volatile("s_setprio 1");   // around the matrix segment only
        __builtin_amdgcn_sched_barrier(0);
        if (!(A6C_ABL & 16)) pv_first();
        __builtin_amdgcn_sched_barrier(0);
        if (!(A6C_ABL & 16)) pv_step(1);
        __builtin_amdgcn_sched_barrier(0);
        if ((steady || req) && !(A6C_ABL & 1)) dma_tile(i + 3, steady);
        __builtin_amdgcn_sched_barrier(0);
        if (!(A6C_ABL & 16)) pv_step(2);
        __builtin_amdgcn_sched_barrier(0);
        const KStep f0 = read_step(i + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (!(A6C_ABL & 16)) pv_step(3);
        __builtin_amdgcn_sched_barrier(0);
        if (!(A6C_ABL & 16)) s_chains(i + 1, f0, steady);
        asm volatile("s_setprio 0");
        A6C_MARK(0);
    };
    // V(t): softmax of tile t -> P, then the V fragments of tile t for the PV that follows in this wave's next M
    auto v_part = [&](int t) __attribute__((always_inline)) {
        if (!(A6C_ABL & 8)) softmax(t);
        __builtin_amdgcn_sched_barrier(0);   // (V reads hoisted above the softmax would hold 32 more registers through it; between the two P
        read_v(t);                           //  conversions they lost 7.5 %, in the matrix segment's issue slots they gained nothing: profiles/r05_attn_d64_ab.txt)
        __builtin_amdgcn_sched_barrier(0);
        A6C_MARK(1);
    };
    auto period_end = [&](bool req) __attribute__((always_inline)) {   // tile i + 2 (requested one period ago) has landed in every wave's view after this barrier
        if (req && !(A6C_ABL & 1)) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        seg_barrier();
        A6C_MARK(2);
    };
    // ---- ONE barrier per 64-key tile.  In a period both halves run one M and one V, in OPPOSITE order:
    //   early half (waves 0..3):  M(t) = PV(t), S(t+1)   then  V(t+1) = softmax(t+1)   | barrier
    //   late half  (waves 4..7):  V(t) = softmax(t)      then  M(t)                    | barrier
    // so that on every SIMD one wave's matrix segment runs beside the other's vector segment without a second barrier (the
    // first version had one between the segments: its release latency was a bubble of the matrix pipe twice per tile).  The
    // barrier is needed for the LDS ring only.  Both halves run the SAME loop body  V(t) [barrier if early] M(t) [barrier if
    // late]: the early half has its first M peeled off in front of the loop, i.e. its loop is rotated by one segment.  (Two
    // loops behind an if / else cost 256 registers + spills where each alone needs ~205; a loop body with ``if (more)`` around
    // the S chains keeps stale sacc / kf / vf values alive -- hence the peeled last PV.  Scratch reloads are not just slow
    // here: they share vmcnt with the LDS-DMA prefetch.)
    // (nt >= 2: the launch code sends single-tile problems to attn_d64b)
    s_chains(0, read_step(0, 0));
    int t = 0;
    if (!late) {
        softmax(0);
        read_v(0);
        seg_barrier();   // the early half enters period 0 one softmax ahead
        m_part(0, 3 < nt);
        t = 1;
    } else {
        seg_barrier();
    }
    if (A6B_STAMP) st_t = a6b_stamp();
    // steady state (tile t + 3 exists and is full): the same body with its five uniform branches per tile folded away -- around
    // the request, its fast / ragged forms, the two ragged-tile masks and the two forms of the counted wait
    for (; t + 4 < nt; ++t) {
        v_part(t);
        if (!late) period_end(true);
        m_part(t, true, true);
        if (late) period_end(true);
    }
    for (; t + 1 < nt; ++t) {
        v_part(t);
        if (!late) period_end(t + 2 < nt);    // closes the period of M(t - 1) (request of tile t + 2), V(t)
        m_part(t, t + 3 < nt);
        if (late) period_end(t + 3 < nt);     // closes the period of V(t), M(t) (request of tile t + 3)
    }
#undef A6C_MARK
    if (A6B_STAMP && p.dbg != nullptr && lane == 0) {
        unsigned long long* d = p.dbg + ((size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + wu) * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = st_sum[i];
        d[5] = (unsigned long long)(nt - 1);
    }
    softmax(nt - 1);
    read_v(nt - 1);
    if (!late) seg_barrier();   // the early half's barrier count: 1 + (nt - 2) + this one = the late half's 1 + (nt - 1)
    pv_first();   // PV of the last tile
    pv_step(1);
    pv_step(2);
    pv_step(3);
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(oacc[0][0]), "+v"(oacc[0][1]), "+v"(oacc[1][0]), "+v"(oacc[1][1]));   // O readable by VALU

    // (O leaves through this wave's own Q image: dead after its last S chain, and private -- the ring may still be read by the
    //  other half's last segments)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float l_tot = l_run[j] + __shfl_xor(l_run[j], 32);
        a6_store_o<T>(Qs + j * 4096, oacc[j], 1.0f / l_tot, q0 + 32 * j, lane, p, b, h);
    }
}
