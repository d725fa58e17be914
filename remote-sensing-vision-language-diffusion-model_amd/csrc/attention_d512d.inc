// Included once by attention.hip (after attn_d512b_kernel): attn_d512d_kernel, the shared-tile (K = V = X) d = 512 kernel with
// O split over the HEAD DIMENSION for the PV product.  Its loop body is attention_d512d_body.inc; the S chain (A5_CHAIN), the Q load
// and the store loops are attention.hip's A5_ macros and the softmax is attention_d512_softmax.inc, the text attn_d512b compiles.
//
// attn_d512b<T, true> lets each of its four waves own 32 query rows over all 512 head dims, so every wave reads the whole 32 KiB
// key tile twice per tile: row-wise for S^T = K Q^T and transposed for O^T += V^T P^T.  Here the S chain and the online softmax
// stay exactly as there (wave w: query rows 32w .. 32w + 31, Q in VGPRs, deferred max), but PV is split by head dimension:
// wave w owns O^T for d in [128w, 128w + 128) across all 128 query rows of the workgroup (4 d-blocks x 4 q-blocks of 32 x 32
// = the same 256 accumulator registers).  Per tile it reads 8 transposed X^T fragments (its own d-slice) instead of 32, and the
// P^T fragments of the three other q-blocks, which every wave publishes in LDS (lane-for-lane: the B operand of another wave's
// q-block has the same lane layout as the wave's own).  Own P^T stays in registers.  The rescale factor alpha of a row travels
// beside P; the final row sums l through LDS once.
//
// LDS per tile and CU: 128 KiB row-wise reads (as before), 32 KiB transposed reads (was 128), 24 KiB P reads + 8 KiB P writes,
// 32 KiB LDS-DMA.  Every O^T element accumulates the same MFMA products (same k order) over the same tiles in the same order,
// with the same alpha and l: the output equals attn_d512b<T, true>'s bit for bit (tests/test_gpu_attn_d512_dsplit.py).
//
// Pipeline (one barrier per tile, as before).  Iteration t:
//   phase A: S(t+1) chain over ring buffer (t+1) & 3 with softmax(t) in its hooks; write P(t), alpha(t) to P buffer t & 1;
//            read this wave's X^T(t) fragments; wait for this wave's LDS-DMA rows; barrier
//   phase B: PV(t) -- own q-block first (its P is in registers), then the three others from LDS -- with the LDS-DMA rows of
//            tile t+3 (-> ring buffer (t+3) & 3 = (t-1) & 3, last read by PV(t-1) before this barrier) between the MFMAs.
// The barrier orders "P(t) written" before "P(t) read"; P(t+2) reuses buffer t & 1 only after the next barrier.  The X ring is
// therefore four deep (X(t) in PV, X(t+1) in S, X(t+2) landed, X(t+3) landing) and the DMA of a tile is waited for one phase A
// after it was issued, as the three-deep ring of attn_d512b waited one PV phase after.
constexpr int A5D_P_OFF = 4 * A5B_TILE;                 // X ring: 4 x 32 KiB
constexpr int A5D_PBUF = 4 * 2 * 64 * 16;               // P(t): 4 waves x 2 k-steps x 64 lanes x 16 B = 8 KiB, two buffers
constexpr int A5D_A_OFF = A5D_P_OFF + 2 * A5D_PBUF;     // alpha(t): [row 0..31][wave] floats, two buffers of 512 B
constexpr int A5D_L_OFF = A5D_A_OFF + 2 * 512;          // final row sums, [row][wave]
constexpr int A5D_SMEM = A5D_L_OFF + 512;               // 145.5 KiB

template <typename T>
__global__ __launch_bounds__(256) void attn_d512d_kernel(AttnArgs p, int keys_per_split, float* part_o, float* part_ml) {
    constexpr int D = 512;
    typedef typename Mfma<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 128 + w * 32;
    const int split = blockIdx.y, nsplit = gridDim.y;
    const int b = blockIdx.z / p.heads, h = blockIdx.z % p.heads;
    const int k_begin = split * keys_per_split;
    const int k_end = min(p.Nk, k_begin + keys_per_split);
    const int nt = (k_end - k_begin + 31) >> 5;
    const T* Qb = (const T*)p.q + (int64_t)b * p.q_bs + (int64_t)h * D;
    const T* Xb = (const T*)p.k + (int64_t)b * p.k_bs + (int64_t)h * D;

    // ---- tile DMA as in attn_d512b (SH image, same swizzle a5b_f): wave w moves key rows 8w .. 8w+7, one 1-KiB row per
    // wave-instruction, M0 declared clobbered (tools/audit_m0.py checks that the compiler never touches M0 in this unit)
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
    // (the lane offsets are formed per request -- one v_xor -- and the row step is scalar: eight offset registers of attn_d512b
    // are what this kernel's phase B needs for its P^T fragments)
    const int64_t x_rowb = p.k_ts * (int64_t)sizeof(T);
    const uint32_t lane16 = (uint32_t)lane << 4;
    const char* x_tile0 = (const char*)(Xb + (int64_t)(k_begin + wu * 8) * p.k_ts);   // + (32 t + i) rows
    auto dma_x = [&](int t, int i) {   // key row 8w+i of tile t -> ring buffer t & 3 (tail tile: rows past Nk re-read the last key)
        const int r = wu * 8 + i;
        const uint32_t dst = lds0 + (t & 3) * A5B_TILE + r * 1024;
        if (k_begin + t * 32 + 32 <= p.Nk) {
            rsvld_lds_dma16_m0(x_tile0 + (int64_t)(t * 32 + i) * x_rowb, lane16 ^ (uint32_t)(a5b_f(r & 15) << 4), dst);
        } else {
            const int key = min(k_begin + t * 32 + r, p.Nk - 1);
            rsvld_lds_dma16_m0((const char*)(Xb + (int64_t)key * p.k_ts), lane16 ^ (uint32_t)(a5b_f(r & 15) << 4), dst);
        }
    };
    auto dma_x_fast = [&](int t, int i) {
        const int r = wu * 8 + i;
        rsvld_lds_dma16_m0(x_tile0 + (int64_t)(t * 32 + i) * x_rowb, lane16 ^ (uint32_t)(a5b_f(r & 15) << 4), lds0 + (t & 3) * A5B_TILE + r * 1024);
    };
#pragma unroll
    for (int i = 0; i < 8; ++i) dma_x(0, i);
    if (nt > 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dma_x(1, i);
    }
    if (nt > 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dma_x(2, i);
    }

    // ---- Q fragments (B operand of S^T: col = query row on the lane, k = d)
    const int qrow = q0 + l31;
    v8 qf[32];
    A5_LOAD_Q(qf)
    // O^T: oacc[dt][j] = d-block 4w + dt (rows d = 128w + 32dt + ..) x q-block (w + j) & 3 (j = 0: this wave's own rows).
    // The q-block is rotated by w so that every register index is a compile-time constant.
    f32x16 oacc[4][4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][j][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // K (row-wise read) of chunk 2c + lh: l31 * 1024 + (((2c + lh) ^ f(l31)) << 4) = kb ^ (c << 5) (one register, not eight)
    const uint32_t kb = l31 * 1024 + ((lh ^ a5b_f(l31 & 15)) << 4);
    // transposed X^T reads of d-block 4w + f: off = buffer + vbase[f] + 256 w + 1024 (16 s + 8 hf) (see attn_d512b)
    int vbase[4];
    {
        const int qq = (lane >> 2) & 3, pp = lane & 3, g1 = (lane >> 4) & 1;
#pragma unroll
        for (int f = 0; f < 4; ++f) vbase[f] = (4 * lh + qq) * 1024 + ((f ^ qq) << 6) + (((2 * g1 + (pp >> 1)) ^ lh) << 4) + ((pp & 1) << 3) + wu * 256;
    }
    auto vread = [&](int buf, int f, int s2) {
        const int off = buf * A5B_TILE + vbase[f] + (16 * s2) * 1024;
        return tr16_pair<v8>(lds_read_tr16(smem + off), lds_read_tr16(smem + ((off ^ 32) + 8 * 1024)));
    };
    // P / alpha exchange addresses: this wave's slot, and q-block (w + j) & 3's
    const int p_own = A5D_P_OFF + wu * 2048 + lane * 16, a_own = A5D_A_OFF + l31 * 16 + wu * 4;
    int p_oth[3], a_oth[3];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        p_oth[j - 1] = A5D_P_OFF + ((wu + j) & 3) * 2048 + lane * 16;
        a_oth[j - 1] = A5D_A_OFF + l31 * 16 + ((wu + j) & 3) * 4;
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // tiles 0, 1, 2 landed

    // ---- S^T chain: attn_d512b's (A5_CHAIN), K fragment c of a k-step group at kb ^ (c << 5)
    uint32_t ka[8];
    v8 kfr[A5_KD];
#define A5_KADDR(KBUF, c) (lds0 + (((KBUF) * A5B_TILE + kb) ^ (c << 5)))
#define A5_KREFILL true

    f32x16 sacc;   // scores of the tile whose softmax is due (S runs one tile ahead of PV)
    if constexpr (__is_same(T, f16)) {
        A5_CHAIN("v_mfma_f32_32x32x16_f16", sacc, 0, A5_NOHOOK);
    } else {
        A5_CHAIN("v_mfma_f32_32x32x16_bf16", sacc, 0, A5_NOHOOK);
    }
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sacc));   // MFMA D -> VALU reader (cdna_hip_programming.md §5.7 item 2)

    int t = 0;
    f32x16 sacc2;
    // steady state, two tiles per trip with the score registers swapping roles (see attention_d512_body.inc): tiles t .. t + 4
    // are full (t + 5 < nt), so neither body tests a bound
#define A5_STEADY 1
#define A5_PAIR 1
    for (; t + 5 < nt;) {
        {
#define S_CUR sacc
#define S_NXT sacc2
#include "attention_d512d_body.inc"
#undef S_CUR
#undef S_NXT
        }
        ++t;
        {
#define S_CUR sacc2
#define S_NXT sacc
#include "attention_d512d_body.inc"
#undef S_CUR
#undef S_NXT
        }
        ++t;
    }
#undef A5_PAIR
#undef A5_STEADY
    for (; t < nt; ++t) {
#define A5_PAIR 0
#define A5_STEADY 0
#define S_CUR sacc
#define S_NXT snext
#include "attention_d512d_body.inc"
#undef S_NXT
#undef S_CUR
#undef A5_STEADY
#undef A5_PAIR
    }
#undef A5_KREFILL
#undef A5_KADDR

    // ---- row sums of every q-block through LDS (a dedicated area: other waves may still read the X ring and P buffers)
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    *(float*)(smem + A5D_L_OFF + l31 * 16 + wu * 4) = l_tot;   // (both half-waves store the same value)
    __syncthreads();
    float inv[4];
    inv[0] = 1.0f / l_tot;
#pragma unroll
    for (int j = 1; j < 4; ++j) inv[j] = 1.0f / *(const float*)(smem + A5D_L_OFF + l31 * 16 + ((wu + j) & 3) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int qr = blockIdx.x * 128 + ((wu + j) & 3) * 32 + l31;
        if (qr >= p.Nq) continue;
        if (nsplit == 1) {
            A5_STORE_ROW(T, (T*)p.out + (int64_t)b * p.o_bs + (int64_t)h * D + (int64_t)qr * p.o_ts + wu * 128, 4, oacc[dt][j], inv[j])
        } else {
            const int64_t row = ((int64_t)split * gridDim.z + blockIdx.z) * p.Nq + qr;
            A5_STORE_ROW(float, part_o + row * D + wu * 128, 4, oacc[dt][j], inv[j])
            if (j == 0 && lh == 0) {   // the row's own wave holds its running max
                part_ml[row * 2] = m_run;
                part_ml[row * 2 + 1] = l_tot;
            }
        }
    }
}
