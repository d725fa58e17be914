// rsvld_plan.h — which kernel runs for a layer, decided in ONE place: the planners of conv_igemm.hip (implicit GEMM), gemm.hip (gemm256),
// conv_halo.hip, norm.hip (GroupNorm) and attention.hip.  Plain host C++: integer arithmetic on a descriptor, no HIP call, no device query, no pointer
// dereference beyond the descriptor (its pointers are compared with NULL only).  Each entry point validates, plans here and launches
// the plan through a flat table of instantiations; rsvld_plan_conv / rsvld_plan_groupnorm / rsvld_plan_attention (include/rsvld_hip.h) hand the same plans to the
// caller, so that nothing outside this header restates a threshold.
#pragma once
#include <stdint.h>
#include "rsvld_hip.h"

namespace rsvld_plan {

// rows (or batch rows) of ONE of the plan_div stacked units: every grid-size test below uses it, so the plan, and with it the order of every
// accumulation, does not depend on how many units share the launch
inline int64_t plan_unit(int64_t n, int plan_div) { return plan_div > 1 ? (n + plan_div - 1) / plan_div : n; }

// K segments per tap of the multi-segment operand forms (RSVLD_F16W1: the pair kernels over ONE segment)
struct Forms {
    bool split, w1, w2, hq;
};
inline Forms forms_of(int dtype) { return {dtype == RSVLD_SPLIT, dtype == RSVLD_F16W1, dtype == RSVLD_F16W2, dtype == RSVLD_F16Q8}; }

// ---------------------------------------------------------------------------------------
// implicit GEMM (conv_igemm.hip): one instantiation of conv_igemm_kernel
// ---------------------------------------------------------------------------------------
struct IgemmPlan {
    int bm, bn, stages, ks;   // tile rows x columns, LDS ring depth, K groups per workgroup
    int reg_staging;          // 0: operands staged by LDS-DMA, 1: through registers (RSVLD_TUNE_REG_STAGING)
};

// Tile choice.  Cout <= 32: 256x32.  Cout <= 64: 128x64 (48 KiB LDS -> 3 workgroups per CU: these layers
// have few K-steps per tile, so co-resident workgroups hide each other's prologue / epilogue).  Otherwise
// 128x128, except when that grid would leave CUs idle (< 256 workgroups): then 64x128 doubles the grid.
// M_plan: the output rows of one planning unit; nk: K steps of 64 channels.
inline IgemmPlan plan_igemm(int64_t M_plan, int Cout, int nk, int tune) {
    const bool glds = !(tune & RSVLD_TUNE_REG_STAGING);
    const int reg = glds ? 0 : 1;
    if (Cout <= 32) return {256, 32, 2, 1, reg};
    const int ov = tune & RSVLD_TUNE_TILE_MASK;
    const int st = glds ? ((tune >> RSVLD_TUNE_STAGES_SHIFT) & 7) : 2;   // the register-staged kernels are double-buffered only
    const bool ksplit = !(tune & RSVLD_TUNE_NO_KSPLIT);
    if (Cout <= 64) {
        if (ov == 1) return {256, 64, 2, 1, reg};
        // measured: 3 WGs/CU x 1 tile in flight (48 KiB) beats 2 WGs/CU x 2 tiles (72 KiB)
        return {128, 64, (st == 3 || st == 4) ? st : 2, 1, reg};
    }
    const int64_t wg128 = ((M_plan + 127) / 128) * ((Cout + 127) / 128);
    const int64_t wg64x128 = ((M_plan + 63) / 64) * ((Cout + 127) / 128);
    // small-M linears (Stage-2 transformer blocks at 16x16 / 32x32 tokens): even 64x128 leaves most CUs idle and
    // the K loop is a latency-bound weight stream.  64x64 tiles double the grid again; 4 x 16 KiB stages keep
    // 3 tiles in flight per workgroup at 2 workgroups per CU.
    if (glds && ov == 0 && wg64x128 < 256) {
        const int64_t wg64 = ((M_plan + 63) / 64) * ((Cout + 63) / 64);
        return {64, 64, 4, (ksplit && st == 0 && wg64 <= 256 && nk >= 16) ? 2 : 1, 0};
    }
    if (ov == 4 || (ov == 0 && wg128 < 256)) {
        if (glds) {
            // one 64x128 workgroup per CU at most and a long K loop: two K groups (8 waves) per tile
            if (ksplit && st == 0 && wg64x128 <= 256 && nk >= 16) return {64, 128, 3, 2, 0};
            if (st == 3 || st == 0) return {64, 128, 3, 1, 0};   // 72 KiB: 2 WGs / CU
            if (st == 4) return {64, 128, 4, 1, 0};
        }
        return {64, 128, 2, 1, reg};
    }
    // measured: the 96 KiB ring drops to 1 WG/CU and loses 30 % to 2 x 64 KiB double buffers
    return {128, 128, (st == 3 || st == 4) ? st : 2, 1, reg};
}

// ---------------------------------------------------------------------------------------
// gemm256 (gemm.hip): large 1x1 / stride-1 / single-source layers
// ---------------------------------------------------------------------------------------
enum { GEMM256_NONE = 0, GEMM256_PERSISTENT = 1, GEMM256_ONE_TILE = 2 };
struct Gemm256Plan {
    int form;        // GEMM256_PERSISTENT: eligible for the persistent kernel (the launch falls back to one tile per workgroup where that
                     // family has no persistent instantiation, or no device tells a CU count); GEMM256_ONE_TILE: one tile per workgroup
    int out_kind;    // 0 = 16-bit (T, or fp16 from the multi-segment forms), 1 = fp32, 2 = bf16 planes (RSVLD_SPLIT's native output)
    bool wide_res;   // fp32 out + fp32 residual, no activation: the persistent form of the multi-segment families
};

// RSVLD_OK: gemm256 takes the layer (*p filled); RSVLD_EUNSUPPORTED: the shape stays on the implicit-GEMM kernel; RSVLD_EINVAL
inline int plan_gemm256(const rsvld_conv_desc* d, Gemm256Plan* p) {
    const Forms f = forms_of(d->dtype);
    const int seg = f.split ? 3 : f.w2 ? 2 : 1;      // K segments (RSVLD_F16W1: one, in the SEG = 4 kernels: the multi-segment family's outputs)
    if (d->tune & RSVLD_TUNE_NO_GEMM256) return RSVLD_EUNSUPPORTED;   // A/B switch
    if (f.w1 && d->out_f32 != 1) return RSVLD_EINVAL;
    if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad_t != 0 || d->pad_l != 0 || d->upsample) return RSVLD_EUNSUPPORTED;
    if (d->x2 != nullptr || d->Cin2 != 0 || d->rowvec != nullptr || (d->out_f32 && seg == 1 && !f.w1)) return RSVLD_EUNSUPPORTED;
    if (d->Cin % 32 != 0 || d->Cout % 8 != 0) return RSVLD_EUNSUPPORTED;
    const int64_t M = (int64_t)d->B * d->Ho * d->Wo;
    if (d->H != d->Ho || d->W != d->Wo) return RSVLD_EUNSUPPORTED;
    const int64_t Mp = plan_unit(M, d->plan_div);
    if (d->Cout < 256 || Mp < 4096) return RSVLD_EUNSUPPORTED;
    const int64_t tiles = ((Mp + 255) / 256) * ((d->Cout + 255) / 256);
    if (tiles < 128) return RSVLD_EUNSUPPORTED;   // one workgroup per CU; measured: from half the chip up it beats the 128x128 kernel
    // 32-bit lane offsets inside a tile: 256 rows of the activation tensor (planes: 2 K per row) / of the weights (pair 2 K, triple 3 K)
    if ((int64_t)256 * d->Cin * 2 * seg >= ((int64_t)1 << 32) || M >= ((int64_t)1 << 31)) return RSVLD_EUNSUPPORTED;
    if (d->act == RSVLD_ACT_GEGLU && (d->Cout % 16 != 0 || d->residual != nullptr)) return RSVLD_EINVAL;
    // RSVLD_SPLIT: the residual is the fp32 stream and goes with the fp32 output only (RSVLD_F16W2: the residual has the output's type)
    if (f.split && d->out_f32 != 1 && d->residual != nullptr) return RSVLD_EINVAL;
    if ((d->out_f32 == 2 && !f.split) || d->out_f32 < 0 || d->out_f32 > 2) return RSVLD_EINVAL;
    p->out_kind = f.w1 ? 1 : seg == 1 ? 0 : d->out_f32 == 1 ? 1 : (f.split && d->out_f32 == 0) ? 2 : 0;
    p->wide_res = (seg > 1 || f.w1) && p->out_kind == 1 && d->residual != nullptr && d->act == RSVLD_ACT_NONE;
    // the persistent form: 16-bit output, at least four K tiles (its K loop peels tile 0 and requests three tiles ahead)
    const bool persistent = !(d->tune & RSVLD_TUNE_GEMM_ONE_TILE) && (p->out_kind == 0 || p->wide_res) && seg * d->Cin >= 128;
    p->form = persistent ? GEMM256_PERSISTENT : GEMM256_ONE_TILE;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// rsvld_conv2d_nhwc: validate -> gemm256 -> implicit GEMM
// ---------------------------------------------------------------------------------------
// K segments the implicit-GEMM kernel walks per tap: RSVLD_SPLIT 3, RSVLD_F16W2 / RSVLD_F16W1 2 (the latter over ONE segment of channels)
inline int igemm_seg(const Forms& f) { return f.split ? 3 : (f.w2 || f.w1) ? 2 : 1; }

// the operand checks of rsvld_conv2d_nhwc, in its order
inline int validate_conv(const rsvld_conv_desc* d) {
    if (d == nullptr || d->x == nullptr || d->w == nullptr || d->out == nullptr) return RSVLD_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0) return RSVLD_EINVAL;
    if (d->Cin <= 0 || d->Cin % 8 != 0 || d->Cout <= 0 || d->Cout % 8 != 0) return RSVLD_EINVAL;
    if (d->Cin2 < 0 || d->Cin2 % 8 != 0 || ((d->Cin2 > 0) != (d->x2 != nullptr))) return RSVLD_EINVAL;
    if (d->KH <= 0 || d->KW <= 0 || d->stride <= 0) return RSVLD_EINVAL;
    // RSVLD_F16W1: the weight-pair kernels (SEG = 2: fp16 in, fp32 out + fp32 residual) over ONE K segment -- their second-segment wrap of the
    // channel index never triggers when Ctot = Cseg, and the weight rows are K long
    const Forms f = forms_of(d->dtype);
    const int seg = igemm_seg(f);
    if (d->dtype != RSVLD_F16 && d->dtype != RSVLD_BF16 && seg == 1) return RSVLD_EINVAL;
    if (f.w1 && (d->out_f32 != 1 || d->KH != 1 || d->KW != 1)) return RSVLD_EINVAL;
    if (d->out_f32 < 0 || d->out_f32 > 2 || (d->out_f32 == 2 && !f.split)) return RSVLD_EINVAL;
    if (seg == 1 && d->out_f32 && (d->Cout > 32 || d->act == RSVLD_ACT_GEGLU || d->residual != nullptr)) return RSVLD_EUNSUPPORTED;
    if (f.split && d->out_f32 != 1 && d->residual != nullptr) return RSVLD_EINVAL;   // planes / fp16 out of RSVLD_SPLIT: no residual (the stream stays fp32)
    if (d->act == RSVLD_ACT_GEGLU && (d->Cout % 16 != 0 || d->residual != nullptr)) return RSVLD_EINVAL;
    if ((int64_t)d->B * d->Ho * d->Wo >= (int64_t)1 << 31) return RSVLD_EUNSUPPORTED;
    if ((int64_t)d->B * d->H * d->W >= (int64_t)1 << 31) return RSVLD_EUNSUPPORTED;
    // every output pixel must read inside the (optionally up-sampled) padded input: shape sanity
    const int Hin = d->upsample ? 2 * d->H : d->H, Win = d->upsample ? 2 * d->W : d->W;
    if ((d->Ho - 1) * d->stride - d->pad_t >= Hin || (d->Wo - 1) * d->stride - d->pad_l >= Win) return RSVLD_EINVAL;
    return RSVLD_OK;
}

// K steps of the implicit-GEMM kernel: 16-byte pieces of 8 channels per tap and segment, 8 pieces per step
inline int igemm_nk(const rsvld_conv_desc* d) {
    const Forms f = forms_of(d->dtype);
    const int Ctot8 = (f.w1 ? 1 : igemm_seg(f)) * ((d->Cin + d->Cin2) / 8);
    return (d->KH * d->KW * Ctot8 + 7) / 8;
}
inline IgemmPlan plan_igemm(const rsvld_conv_desc* d) {   // of a descriptor validate_conv accepted
    const int64_t M = (int64_t)d->B * d->Ho * d->Wo;
    return plan_igemm(plan_unit(M, d->plan_div), d->Cout, igemm_nk(d), d->tune);
}

// ---------------------------------------------------------------------------------------
// halo convolution (conv_halo.hip)
// ---------------------------------------------------------------------------------------
constexpr int HALO_TH = 8, HALO_TW = 32;   // output pixels of a tile; the 8-wave kernel stacks two tiles (16 x 32)
struct HaloPlan {
    int bn, waves;       // output channels per workgroup; 4 waves on an 8 x 32 tile or 8 waves on 16 x 32
    int64_t wgs;         // workgroups of ONE planning unit, on 8-row tiles also where the 8-wave kernel runs
    int stat_tiles;      // 8 x 32 tiles per image: the rows of the epilogue's statistics partials
};

// 3x3 / stride 1 / pad 1, every source a multiple of 64 channels
inline bool halo_supported(const rsvld_conv_desc* d) {
    if (d == nullptr) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1) return false;
    const int up = d->upsample ? 2 : 1;
    if (d->Ho != up * d->H || d->Wo != up * d->W) return false;
    if (d->Cin % 64 != 0 || d->Cin2 % 64 != 0) return false;
    if (d->act == RSVLD_ACT_GEGLU) return false;
    if (d->out_f32 && d->Cout > 32 && d->dtype != RSVLD_SPLIT && d->dtype != RSVLD_F16W2 && d->dtype != RSVLD_F16Q8) return false;
    // RSVLD_F16Q8: the 128-wide kernels only; fp32 out; ONE source (the GroupNorm apply pass that writes q8 rows has already concatenated)
    if (d->dtype == RSVLD_F16Q8 && (d->Cout <= 64 || !d->out_f32 || d->upsample || d->Cin2 != 0)) return false;
    if (d->Wo < 16 || d->Ho < 4) return false;   // tiny maps: the 8x32 tile would be mostly padding
    return true;
}

// K segments per tap the halo kernels walk (RSVLD_F16Q8: SEG = 5, two fp16 segments' worth of weight row)
inline int halo_seg(const Forms& f) { return f.split ? 3 : f.w2 ? 2 : f.hq ? 5 : 1; }

// logical K' channels per tap (16-bit elements of a weight row)
inline int halo_ctot(const rsvld_conv_desc* d) {
    const Forms f = forms_of(d->dtype);
    return (f.hq ? 2 : halo_seg(f)) * (d->Cin + d->Cin2);
}

inline bool plan_halo(const rsvld_conv_desc* d, HaloPlan* p) {
    if (!halo_supported(d)) return false;
    const int64_t B_plan = plan_unit(d->B, d->plan_div);
    const int tiles_x = (d->Wo + HALO_TW - 1) / HALO_TW;
    p->stat_tiles = tiles_x * ((d->Ho + HALO_TH - 1) / HALO_TH);
    if (d->Cout <= 64) {
        p->bn = 64, p->waves = 4;
    } else {
        // 16x32-pixel tiles (one 8-wave workgroup per CU) once that grid still covers most of the chip
        const int64_t wg16 = (int64_t)tiles_x * ((d->Ho + 2 * HALO_TH - 1) / (2 * HALO_TH)) * B_plan * ((d->Cout + 127) / 128);
        // measured (tools/bench_halo.py, one box): +3..13 % from 192 channels of K up, -3 % at 128 (longer pipeline fill)
        const bool use8 = (d->tune & RSVLD_TUNE_HALO_NW8) ? true : (d->tune & RSVLD_TUNE_HALO_NW4) ? false : (wg16 >= 192 && halo_ctot(d) >= 192);
        p->bn = 128, p->waves = use8 ? 8 : 4;
    }
    p->wgs = B_plan * p->stat_tiles * ((d->Cout + p->bn - 1) / p->bn);
    return true;
}

// ---------------------------------------------------------------------------------------
// the whole plan of a convolution descriptor (rsvld_plan_conv)
// ---------------------------------------------------------------------------------------
inline int plan_conv(const rsvld_conv_desc* d, rsvld_conv_plan* out) {
    *out = rsvld_conv_plan{};
    HaloPlan h;
    if (plan_halo(d, &h)) out->halo_wgs = h.wgs, out->halo_bn = h.bn, out->halo_waves = h.waves, out->halo_stat_tiles = h.stat_tiles;
    int rc = validate_conv(d);
    if (rc != RSVLD_OK) return rc;
    Gemm256Plan g;
    rc = plan_gemm256(d, &g);
    if (rc == RSVLD_OK) {
        out->gemm256 = g.form;
        return RSVLD_OK;
    }
    if (rc != RSVLD_EUNSUPPORTED) return rc;
    const IgemmPlan p = plan_igemm(d);
    out->bm = p.bm, out->bn = p.bn, out->stages = p.stages, out->ks = p.ks, out->reg_staging = p.reg_staging;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// GroupNorm (norm.hip)
// ---------------------------------------------------------------------------------------
constexpr int GN_SMALL_MAXV = 32;   // sixteen-byte vectors a thread of gn_small_kernel holds

// threads per row of gn_partial_kernel over C8 eight-channel vectors; 256 / that = its rows in flight
constexpr int gn_threads_per_row(int C8) { return C8 < 256 ? C8 : 256; }

// one workgroup per (image, group) with the group's slab in registers: 8 | C/groups (a vector never straddles groups), groups that
// do not straddle the two sources, at most GN_SMALL_MAXV vectors per thread
inline bool gn_small_ok(int HW, int C1, int C2, int groups) {
    const int C = C1 + C2, gs = C / groups;
    if (gs % 8) return false;
    const int gs8 = gs / 8;
    if (gs8 > 256 || (gs8 & (gs8 - 1))) return false;
    if (C2 > 0 && C1 % gs) return false;
    if ((int64_t)HW * gs8 > (int64_t)256 * GN_SMALL_MAXV) return false;
    // (the choice must not depend on the batch: batch-invariant results)
    return groups >= 32;       // enough workgroups per image to be worth one launch
}

struct GnPlan {
    int nchunks, rows_per_chunk;
};
// the row chunks of the partials route.  The chunking fixes the order of the partial sums: it depends on the image size only, so an
// image's statistics are bit-identical whatever the batch around it
inline GnPlan gn_plan(int HW) {
    const int max_chunks = 512;
    int rpc = (HW + max_chunks - 1) / max_chunks;
    if (rpc < 64) rpc = 64;
    return {(HW + rpc - 1) / rpc, rpc};
}

// operand checks of the GroupNorm entry points: the sizes of [x (C1) | x2 (C2)] and the groups over C1 + C2
inline bool gn_dims_ok(int B, int HW, int C1, int C2) { return B > 0 && HW > 0 && C1 > 0 && C1 % 8 == 0 && C2 >= 0 && C2 % 8 == 0; }
inline bool gn_groups_ok(int C, int groups) { return groups > 0 && C % groups == 0 && C <= 8192 && groups <= 256; }

// the one-workgroup route of rsvld_groupnorm_nhwc / rsvld_groupnorm_scale_shift: 16-bit inputs, a grid of (groups, B)
inline bool gn_small_route(int dtype, int B, int HW, int C1, int C2, int groups) {
    return (dtype == RSVLD_F16 || dtype == RSVLD_BF16) && B <= 65535 && gn_small_ok(HW, C1, C2, groups);
}

inline int plan_groupnorm(int dtype, int B, int HW, int C1, int C2, int groups, rsvld_groupnorm_plan* out) {
    *out = rsvld_groupnorm_plan{};
    if (!gn_dims_ok(B, HW, C1, C2) || !gn_groups_ok(C1 + C2, groups)) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16 && dtype != RSVLD_F32) return RSVLD_EINVAL;
    const GnPlan pl = gn_plan(HW);
    out->small = gn_small_route(dtype, B, HW, C1, C2, groups) ? 1 : 0;
    out->nchunks = pl.nchunks, out->rows_per_chunk = pl.rows_per_chunk;
    out->rows_in_flight = 256 / gn_threads_per_row((C1 + C2) / 8);
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// attention (attention.hip): the kernel, its grid, the split-KV ranges and the workspace of one launch
// ---------------------------------------------------------------------------------------
typedef rsvld_attention_plan AttnPlan;

// 8 waves (256 query rows) of attn_d64b share each K / V tile from this many query rows on; the gain is small
#ifndef A6B_NW8_MIN
#define A6B_NW8_MIN 16384   // round 2 (one box, 2 x 10 heads): +1.5 % at 65 536 tokens, -0.5 % (noise) at 16 384; with the bias step
                            // (round 3, 2 x 20 heads at 16 384 tokens): +1.3 % (880 -> 891 TFLOP/s), so 16 384 tokens take it too
#endif
#ifndef A6C_MIN_WG
#define A6C_MIN_WG 1024   // the ping-pong kernel is used when its grid (512 query rows per workgroup, one workgroup per CU) has at
#endif                    // least this many workgroups (4 rounds of the 256 CUs): measured +2.3 % at 2 x 20 heads x 16 384 tokens (1 280
                          // workgroups), +4.5 % at 2 x 10 x 65 536 (2 560); 25 % SLOWER at 2 x 10 x 4 096 (160 workgroups)
#ifndef A6C_MIN_KEYS
#define A6C_MIN_KEYS 512   // ... and at least this many keys: on the 77-key cross-attention of the same token counts attn_d64b is faster
#endif                     // (70 vs 89 us at 2 x 20 x 16 384 queries, 158 vs 178 at 2 x 10 x 65 536: prologue and tail are all there is)
// split-KV plan of the D = 512 kernels: key ranges per workgroup
//   (a) so that the grid fills the 256 CUs when the query tiles alone cannot;
//   (b) so that ONE key range stays resident in the 256 MiB Infinity Cache while every query tile streams it.  At
//       N = 262 144 the key/value tensor is 268 MB (shared tile) or 537 MB: every workgroup re-streamed it from HBM
//       (rocprofv3 FETCH_SIZE: ~400 GB per launch, ~3 TB/s for the whole 131 ms).  Workgroups are dispatched range-major
//       (blockIdx.y), so with ranges of A5B_MALL_KEYS keys (64 MiB shared / 128 MiB as two tensors) all the query tiles in
//       flight read the same range out of the cache; the price is one fp32 partial (O, m, l) per range and the merge pass.
//       Measured on one box (N = 262 144, shared tile): 1036 TFLOP/s with 64 Ki-key ranges, 1041 without, 1026 with 32 Ki:
//       the kernel is NOT bound by that HBM stream (its LDS-DMA requests are two tiles ahead), so this buys no time; it is
//       kept because it takes ~3 TB/s of needless HBM traffic (and its power) out of the dominant Stage-1 kernel.
#ifndef A5B_MALL_KEYS
#define A5B_MALL_KEYS 65536
#endif

// shared: keys and values are ONE tensor (same pointer and strides); k_ts / v_ts: the token strides of k and v in elements (D = 64 only).
// RSVLD_OK with *p filled; RSVLD_EINVAL / RSVLD_EUNSUPPORTED as rsvld_attention_tuned returns them for these arguments
inline int plan_attention(int B, int heads, int Nq, int Nk, int D, int plan_div, int tune, bool shared, int64_t k_ts, int64_t v_ts, AttnPlan* p) {
    *p = AttnPlan{};
    if (B <= 0 || heads <= 0 || Nq <= 0 || Nk <= 0 || heads > 65535 || B > 65535) return RSVLD_EINVAL;
    if (D == 512) {
        // the key split (an accumulation-order choice) is planned on ONE of the plan_div stacked units
        const int64_t base = (int64_t)((Nq + 127) / 128) * plan_unit(B, plan_div) * heads;
        int ns = 1;
        if (base < 192) {
            ns = (int)((256 + base - 1) / base);
            const int cap = Nk / 256 > 1 ? Nk / 256 : 1;   // at least 8 key tiles per range
            if (ns > cap) ns = cap;
            if (ns > 16) ns = 16;
        }
        if (A5B_MALL_KEYS > 0 && Nk > A5B_MALL_KEYS + A5B_MALL_KEYS / 2) {
            const int nm = (Nk + A5B_MALL_KEYS - 1) / A5B_MALL_KEYS;
            if (nm > ns) ns = nm;
        }
        p->keys_per_split = ((Nk + ns - 1) / ns + 31) / 32 * 32;
        p->nsplit = (Nk + p->keys_per_split - 1) / p->keys_per_split;
        if (p->nsplit > 1) p->ws_bytes = (int64_t)p->nsplit * B * heads * Nq * (512 + 2) * 4;   // fp32 partials (O | m, l) per range
        // shared tile: the head-dimension split of PV (attn_d512d) unless tune asks for the row-owning form; the two agree bit
        // for bit (tests/test_gpu_attn_d512_dsplit.py)
        p->row = !shared ? RSVLD_ATTN_ROW_D512B : tune == RSVLD_ATTN_D512_ROWS ? RSVLD_ATTN_ROW_D512B_SHARED : RSVLD_ATTN_ROW_D512D;
        p->grid_x = (Nq + 127) / 128, p->grid_y = p->nsplit, p->grid_z = B * heads;
        return RSVLD_OK;
    }
    if (D != 64) return RSVLD_EUNSUPPORTED;
    // tune (RSVLD_ATTN_D64_*: tests and A/B runs) overrides the choice between the two d = 64 kernels, which agree bit for
    // bit on every shape; 0 = by grid size
    const char force = tune == RSVLD_ATTN_D64_FOUR_WAVE ? 'b' : tune == RSVLD_ATTN_D64_PINGPONG ? 'c' : 0;
    const int64_t wg_c = (int64_t)((Nq + 511) / 512) * heads * B;
    // attn_d64c forms 32-bit lane offsets of up to 64 key rows: a token stride of ~16 M elements or more would wrap
    const bool c_strides_ok = 64 * k_ts * 2 < ((int64_t)1 << 32) && 64 * v_ts * 2 < ((int64_t)1 << 32);
    if (force == 'c' && !c_strides_ok) return RSVLD_EUNSUPPORTED;
    p->nsplit = 1, p->keys_per_split = Nk;
    int rows = 128;
    if (c_strides_ok && force != 'b' && Nk > 64 && ((wg_c >= A6C_MIN_WG && Nk >= A6C_MIN_KEYS) || force == 'c'))
        p->row = RSVLD_ATTN_ROW_D64C, rows = 512;         // long query sequences: the ping-pong kernel
    else if (Nq >= A6B_NW8_MIN)
        p->row = RSVLD_ATTN_ROW_D64B_NW8, rows = 256;     // long query sequences: 8 waves (256 query rows) share each K / V tile
    else
        p->row = RSVLD_ATTN_ROW_D64B_NW4;
    p->grid_x = (Nq + rows - 1) / rows, p->grid_y = heads, p->grid_z = B;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// causal grouped-query prefill attention (prefill_attention.hip): rows are (position, head-in-group) pairs of one kv head, T g of them,
// 128 per workgroup (4 waves x 32); grid = (row blocks, kv heads), no key split and no workspace.  A function of (T, n_q, n_kv) alone:
// pos0 and max_len change how many key tiles a workgroup walks, never which rows it owns.
// ---------------------------------------------------------------------------------------
constexpr int PREFILL_ATTN_ROWS = 128;   // rows per workgroup
constexpr int PREFILL_ATTN_KEYS = 64;    // keys per tile (tiles start on absolute multiples of it)
inline int plan_prefill_attention(int T, int n_q, int n_kv, int head_dim, rsvld_prefill_attention_plan* p) {
    *p = rsvld_prefill_attention_plan{};
    if (T < 1 || n_q < 1 || n_kv < 1 || n_q % n_kv != 0 || n_kv > 65535) return RSVLD_EINVAL;
    const int g = n_q / n_kv;
    if (head_dim != 128 || g > 8) return RSVLD_EUNSUPPORTED;
    if ((int64_t)T * g > ((int64_t)1 << 30)) return RSVLD_EINVAL;   // the kernel's 32-bit row index
    p->rows_per_wg = PREFILL_ATTN_ROWS, p->keys_per_tile = PREFILL_ATTN_KEYS;
    p->grid_x = (int32_t)(((int64_t)T * g + PREFILL_ATTN_ROWS - 1) / PREFILL_ATTN_ROWS), p->grid_y = n_kv;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// the decode-step attention on MFMAs (dam_kernel of decode_attention.hip): a workgroup owns (sequence, kv head, one range of DAM_RANGE keys on
// absolute boundaries); its DAM_WAVES waves take DAM_RANGE / DAM_WAVES consecutive keys each.  DAM_RANGE is a constant -- no function
// of the number of sequences, of max_len or of a position -- so the key order of a sequence's sum is the same in every call; max_len
// only decides how many ranges there are (those above the position write neutral partials).  The number of sequences is no argument.
// ---------------------------------------------------------------------------------------
constexpr int DAM_RANGE = 128, DAM_WAVES = 4, DAM_TILE_KEYS = 64;
constexpr int DAM_LDS_BYTES = 2 * DAM_RANGE * 128 * 2;   // K and V of the range, 16-bit
static_assert(DAM_RANGE % 64 == 0 && DAM_RANGE % DAM_TILE_KEYS == 0 && DAM_RANGE / DAM_WAVES == 32, "a wave takes one 32-key MFMA block");
inline int plan_decode_attention_mma(int n_q, int n_kv, int max_len, int dtype, rsvld_decode_attention_mma_plan* p) {
    *p = rsvld_decode_attention_mma_plan{};
    if (n_q < 1 || n_kv < 1 || max_len < 1 || n_q % n_kv != 0 || n_kv > 65535) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (n_q / n_kv > 8) return RSVLD_EUNSUPPORTED;
    const int64_t ranges = ((int64_t)max_len + DAM_RANGE - 1) / DAM_RANGE;
    if (ranges > 65535) return RSVLD_EUNSUPPORTED;                            // grid_y
    p->range_keys = DAM_RANGE, p->ranges = (int32_t)ranges, p->waves = DAM_WAVES, p->lds_bytes = DAM_LDS_BYTES;
    p->grid_x = n_kv, p->grid_y = (int32_t)ranges;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// 16-bit rows x e4m3 packs (gemm_w8.hip): ONE tile shape, ONE K order (ascending steps of GW_BK, no split over K), whatever the shape
// is -- so there is nothing here that M could move: it enters grid_x alone, and a row's bits do not depend on the rows around it.
// Grid = (row tiles, column tiles): the row tiles of one column tile are dispatched together and share its weight bytes in L2.
// ---------------------------------------------------------------------------------------
constexpr int GW_BM = 128, GW_BN = 128, GW_BK = 64, GW_WAVES = 4;
inline int plan_gemm_w8(int M, int N, int K, int dtype, rsvld_gemm_w8_plan* p) {
    *p = rsvld_gemm_w8_plan{};
    if (M < 1 || N < 1 || K < 1) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (K % 16 != 0) return RSVLD_EUNSUPPORTED;                               // 16-byte pieces of e4m3
    if (((int64_t)N + GW_BN - 1) / GW_BN > 65535) return RSVLD_EUNSUPPORTED;  // grid_y
    p->tile_m = GW_BM, p->tile_n = GW_BN, p->tile_k = GW_BK, p->waves = GW_WAVES;
    p->grid_x = (int32_t)(((int64_t)M + GW_BM - 1) / GW_BM), p->grid_y = (N + GW_BN - 1) / GW_BN;
    return RSVLD_OK;
}

// ---------------------------------------------------------------------------------------
// the decode products on MFMAs (gemv_mma.hip): a wave streams GM_ROWS weight rows in steps of GM_STEP_BYTES per row through its own LDS
// slab into the A operand of 16x16x32 MFMAs.  The route -- K split or not, its ways, the step and the slab -- is a function of
// (N, K, weight kind) ONLY.  The number of activation rows is no argument: it decides how many rows are staged and in how many
// launches they go (group_rows, a function of K), never the order a row's sum is taken in.
// Row route: a wave owns a block of GM_ROWS output rows over all of K, a workgroup GM_WAVES blocks.  K-split route (few row blocks: the
// row route would leave most of a 256-CU chip idle; and at least two steps per wave to split): the GM_WAVES waves of a workgroup take
// consecutive ranges of whole steps of ONE block and their partial sums meet in LDS in wave order.
// ---------------------------------------------------------------------------------------
constexpr int GM_ROWS = 16, GM_WAVES = 4, GM_STEP_BYTES = 512;
constexpr int GM_SLAB = GM_ROWS * GM_STEP_BYTES;                       // bytes of one wave's slab
constexpr int GM_LDS = 160 * 1024, GM_PART = GM_WAVES * GM_ROWS * 16 * 4, GM_SCRATCH = 64;
// bytes between two staged rows: K elements, rounded up to the 256 bytes of the LDS bank row, plus 32 -- the rows a quarter-wave reads
// as the B operand then fall into different banks
constexpr int64_t gm_xstride(int K) { return ((int64_t)K * 2 + 255) / 256 * 256 + 32; }
inline int plan_gemv_mma(int N, int K, int w8, int dtype, rsvld_gemv_mma_plan* p) {
    *p = rsvld_gemv_mma_plan{};
    if (N < 1 || K < 1) return RSVLD_EINVAL;
    if (dtype != RSVLD_F16 && dtype != RSVLD_BF16) return RSVLD_EINVAL;
    if (K % (w8 ? 16 : 8) != 0 || (int64_t)K * 2 + 128 > 65536) return RSVLD_EUNSUPPORTED;   // (K's limit in gv_check, gemv_fused.h)
    p->step_k = w8 ? GM_STEP_BYTES : GM_STEP_BYTES / 2;
    p->slab_bytes = GM_SLAB;
    p->rows_per_block = GM_ROWS;
    const int steps = (K + p->step_k - 1) / p->step_k;
    p->ksplit = (steps >= 2 * GM_WAVES && ((int64_t)N + GM_WAVES * GM_ROWS - 1) / (GM_WAVES * GM_ROWS) < 256) ? 1 : 0;
    p->ways = p->ksplit ? GM_WAVES : 1;
    p->steps_per_way = (steps + p->ways - 1) / p->ways;
    p->blocks = (int32_t)(p->ksplit ? ((int64_t)N + GM_ROWS - 1) / GM_ROWS : ((int64_t)N + GM_WAVES * GM_ROWS - 1) / (GM_WAVES * GM_ROWS));
    const int64_t fit = (GM_LDS - GM_WAVES * GM_SLAB - GM_PART - GM_SCRATCH) / gm_xstride(K);   // >= 1: a row is < 64 KiB + 288
    p->group_rows = (int32_t)(fit < RSVLD_DECODE_MAX_ROWS ? fit : RSVLD_DECODE_MAX_ROWS);
    return RSVLD_OK;
}

}  // namespace rsvld_plan
