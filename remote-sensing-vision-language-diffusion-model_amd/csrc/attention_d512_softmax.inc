// Included inside the `sm` lambda (auto sm = [&](int part) { .. }) of both d = 512 loop bodies, attention_d512_body.inc (attn_d512b)
// and attention_d512d_body.inc (attn_d512d): the online softmax of tile t on the scores S_CUR, register-local (this lane holds 16 of
// its query's 32 scores, lane ^ 32 the rest), cut into parts 0..6 for the hooks of the S(t + 1) chain.  Shared as TEXT: as a
// __forceinline__ function over references every d = 512 kernel grew by ~50 instructions (profiles/shared_primitives_isa.txt).
// Takes S_CUR, A5_STEADY (1: the tile is known to be full, no ragged mask) and the body's mx, alpha, rs, need, pf, m_run, l_run.
// Each part ends with an empty volatile asm naming what it produced: volatile asms keep their order, so the part is computed at its
// hook; without the pins hipcc sinks the whole softmax behind the chain.
            if (part == 0) {
                if (!A5_STEADY && k_begin + (t + 1) * 32 > k_end) {   // ragged last tile (uniform branch)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kv = k_begin + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (kv >= k_end) S_CUR[r] = -INFINITY;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S_CUR[r]);   // on the raw scores: scale > 0 commutes with max
                asm volatile("" : "+v"(S_CUR), "+v"(mx));
            } else if (part == 1) {
                mx = a5b_halfwave_max(mx) * p.scale_log2e;
                // deferred max (T13): the reference point moves only when the tile max exceeds it by more than 2^8, so
                // the rescale of O (256 accumulator registers through VGPRs) is skipped on almost every tile
                need = mx > m_run + A5_DEFER_LOG2;   // true on the first tile (m_run = -inf)
                if (need) {
                    alpha = __builtin_amdgcn_exp2f(m_run - mx);
                    m_run = mx;
                }
                asm volatile("" : "+v"(alpha), "+v"(m_run));
            } else if (part >= 2 && part <= 5) {
                const int r0 = 4 * (part - 2);
#pragma unroll
                for (int r = r0; r < r0 + 4; ++r) {
                    S_CUR[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(S_CUR[r], p.scale_log2e, -m_run));   // one fma: no scale pass
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
