// attention_d128.h -- the K / V tile core of the caption's two d = 128 MFMA attentions (prefill_attn_d128_kernel of prefill_attention.hip,
// dam_kernel of decode_attention.hip): workgroups of four waves, tiles of 64 keys x 128 d (16-bit) filled by LDS-DMA alone, S^T = K Q^T with
// the keys on the accumulator registers and the query on the lane, O^T += V^T P^T.  Each kernel keeps its own tile walk, softmax and merge.
//
// An LDS tile is 64 rows of 16 chunks of 16 bytes, XOR-swizzled on the DMA's SOURCE side (the lane picks which source chunk lands in its slot):
//   K: chunk `pos` of row r holds source chunk pos ^ (r & 15): the 16 rows of a ds_read_b128 wavefront quarter land in 16 distinct 16-byte
//      positions of the 256-byte bank period;
//   V: chunk `pos` of row r holds source chunk pos ^ ((r & 3) << 2): the four rows of a transposed read (ds_read_b64_tr_b16) land in four
//      distinct 64-byte quarters.
#pragma once
#include "rsvld_common.h"
typedef short s16x8 __attribute__((__vector_size__(8 * sizeof(short))));
constexpr int A128_TILE = 64 * 256;   // bytes of a tile: 64 keys x 128 d, 16-bit

// ---- tile DMA.  Wave w moves key rows 16 w .. 16 w + 15 of a tile: 4 wave-instructions of 4 rows x 256 B per tensor (rsvld_lds_dma16 /
// _addr: M0, the LDS destination, saved and restored).  Lane (row = lane >> 4, pos = lane & 15) of piece i fills chunk `pos` of the wave's
// row rr = 4 i + row with the source chunk at these byte offsets of its key row.  No key above the kernel's last one is requested: a row
// above it re-reads that key; its score is masked and its V row zeroed in the fragment registers.  (The two loops stay in the kernels:
// as one function here they changed both instruction streams, and prefill_attn_d128_kernel measured 0.4 % slower against a
// parent-vs-parent spread of 0.3 %: profiles/caption_attention_core_ab.txt.)
__device__ __forceinline__ int a128_k_swz(int lane, int rr) { return ((lane & 15) ^ rr) << 4; }
__device__ __forceinline__ int a128_v_swz(int lane, int rr) { return ((lane & 15) ^ ((rr & 3) << 2)) << 4; }

// ---- Q fragments (B operand: col = the query on the lane, k = d = 16 ks + 8 lh ..).  a128_pin_q consumes them and waits for every load
// and DMA piece in flight: hipcc's wait for the Q loads then does not land inside the code that follows (see attn_d64b).
template <typename T>
__device__ __forceinline__ void a128_load_q(const T* Qr, int lh, typename Mfma<T>::v8 (&qf)[8]) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = __builtin_bit_cast(typename Mfma<T>::v8, *(const u32x4*)(Qr + ks * 16 + lh * 8));
}
template <typename V8>
__device__ __forceinline__ void a128_pin_q(V8 (&qf)[8]) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- K fragment (A operand of S^T, ds_read_b128): byte offset of row l31 of a 32-key half, chunk 2 ks + lh, swizzled by row & 15
__device__ __forceinline__ int a128_k_off(int l31, int lh, int ks) { return l31 * 256 + (((2 * ks + lh) ^ (l31 & 15)) << 4); }
// ---- the key, within its 32-key half, of accumulator register r of S^T (and, for r < 8, of element r of a 16-key P / V fragment)
__device__ __forceinline__ int a128_key(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }
// ---- V fragment (A operand of O^T, row = d, k = key in P's register order), transposed read (ds_read_b64_tr_b16, twice: rows + 8 lie 2048
// bytes on): lane 16 g1 + 4 qq + pp supplies row 8 hf + 4 lh + qq of a 16-key group, d = 32 dt + 16 (g1 & 1) + 4 pp .. + 3, at byte
// (4 lh + qq) * 256 + ((dt ^ qq) << 6) + ((2 g1 + (pp >> 1)) << 4) + ((pp & 1) << 3) of the group; element j of the fragment is key
// a128_key(j, lh) of the group.  The offset and the zeroing of the keys above a limit (0 x NaN would be NaN) stay in the kernels: as
// functions here the zeroing loop made prefill_attn_d128_kernel 4.4 - 6.8 % slower, with FEWER instructions
// (profiles/caption_attention_core_ab.txt), and the offset made dam_kernel 46 instructions longer (1216 -> 1262, cross-compiled).
