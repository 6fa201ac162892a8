// The main loop's shared pieces of the W-direct row-owning kernels (rowgemm_wd_kernel, rowgemm_wa_kernel, rowffn_kernel,
// rowblock_kernel, rowres_kernel, rowconv_wd_kernel, hiftconv_kernel, hiftpair_kernel), in ONE place: the weight-fragment
// register buffer, the fp16x3 MFMA triple and the A-fragment read.  As in row_tail.h the pieces take and return values or
// references; addresses, the weight walkers (advance_w, quad_ptrs) and the PLACE of every load, counted wait and barrier stay
// in the kernels, each of which keeps the order it chose and the derivation of its own wait count.  (The vocoder's two,
// hiftconv_kernel and hiftpair_kernel, were one text twice: their walker and step are shared a level up, in hift_common.h.)
#pragma once
#include "row_tail.h"

namespace jv {

// ---- the weight-fragment register buffer: NB steps of lookahead x 2 column blocks x 2 fp16 planes ----
// Loaded and waited for by hand: left to the compiler, the wait in front of a step's first MFMA becomes s_waitcnt vmcnt(0)
// -- its bookkeeping gives up on loads carried around the loop -- and the lookahead is gone.  The asm load is invisible to
// that bookkeeping, so the buffer is sound only under three rules:
//   (a) nothing but the MFMAs may read q[][][], and only behind a fence: the kernel's counted s_waitcnt is followed by
//       landed_mid() / landed_all(), whose "+v" operands order every later read of those registers behind the wait;
//   (b) the register allocator must not copy or spill q while a load is in flight in it (it cannot know one is): one
//       unrolled loop body, no peeled copies of it -- tools/check_rowgemm_isa.py checks the built code object for (a) and (b);
//   (c) every step issues its loads unconditionally; past the end of the launch the kernel's walker wraps around to weights
//       that exist, the loads land where nothing reads them, and the kernel ends with vmcnt(0) + landed_all(): the registers
//       stay reserved until then.
// zero() gives the "+v" operands of the first loads a defined value.
// The two asm statements: WFragBuf's members, and called directly by the one kernel that keeps the eight registers as a
// plain array under the same rules (rowffn_kernel: as a struct its phase loops gain two s_waitcnt at tile height 4):
__device__ __forceinline__ void wfrag_load(rg_u32x4& dst, const unsigned short* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void wfrag_landed(rg_u32x4& b00, rg_u32x4& b01, rg_u32x4& b10, rg_u32x4& b11) {
  asm volatile("" : "+v"(b00), "+v"(b01), "+v"(b10), "+v"(b11)::"memory");
}
template <int NB = 2>
struct WFragBuf {
  rg_u32x4 q[NB][2][2];      // [buffer = step % NB][column block nt][plane]
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 4 * NB; ++i) q[i >> 2][(i >> 1) & 1][i & 1] = rg_u32x4{0u, 0u, 0u, 0u};
  }
  // plane pl of column block nt of a step into buffer b.  (One plane per call: the kernel forms the second address behind the
  // first load, as it always did -- with both addresses as arguments both are live across the first load: two VGPRs more)
  template <int b, int nt, int pl>
  __device__ __forceinline__ void load(const unsigned short* p) {
    wfrag_load(q[b][nt][pl], p);
  }
  // behind the counted wait in the middle of the step that multiplies buffer b: its block 1 and the next step's block 0
  template <int b>
  __device__ __forceinline__ void landed_mid() {
    constexpr int n = (b + 1) % NB;
    wfrag_landed(q[b][1][0], q[b][1][1], q[n][0][0], q[n][0][1]);
  }
  // behind vmcnt(0): after the prologue, and after the last step's wrapped-around loads
  __device__ __forceinline__ void landed_all() {
#pragma unroll
    for (int b = 0; b < NB; ++b) wfrag_landed(q[b][0][0], q[b][0][1], q[b][1][0], q[b][1][1]);
  }
};

// ---- fp16x3: acc + (a_hi + a_lo)(b_hi + b_lo) without the lo lo term, smallest terms first (as the tile kernels do) ----
// NP = 1 (the estimator's FP16 mode, EstRoute::np): the hi hi product alone.  The kernels load, wait and fence exactly as at
// NP = 3 -- the lo planes of the weight fragments still arrive in WFragBuf and are simply not multiplied, so the three rules
// above and every kernel's wait derivation hold unchanged.  The vocoder's kernels take the default.
template <int NP = 3>
__device__ __forceinline__ rg_f32x4 h3_mma(rg_f32x4 acc, const rg_u32x4& a_hi, const rg_u32x4& a_lo, const rg_u32x4& b_hi, const rg_u32x4& b_lo) {
  static_assert(NP == 3 || NP == 1, "three products or the hi hi product alone");
  if constexpr (NP == 3) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(rg_f16x8, a_lo), __builtin_bit_cast(rg_f16x8, b_hi), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(rg_f16x8, a_hi), __builtin_bit_cast(rg_f16x8, b_lo), acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(rg_f16x8, a_hi), __builtin_bit_cast(rg_f16x8, b_hi), acc, 0, 0, 0);
}

// ---- A fragments out of LDS ----
// 16-byte slot key of a row inside its 16-row group: with 64-byte rows (32 fp16), lane l of a 16x16x32 fragment read
// takes row l & 15, k-slot l >> 4; XOR-ing bit 1 of the slot with bit 2 of the row puts the 16 lanes of every
// ds_read_b128 lane group on 16 distinct 16-byte bank slots (brute-forced over the four lane groups of MI355X_MICROARCH.md)
__device__ __forceinline__ int rg_key(int r) { return ((r >> 2) & 1) << 1; }
// byte offset of k-slot kq of row `row` inside a plane: the slot alone, and with the row's 64 bytes
__device__ __forceinline__ int afrag_slot(const int row, const int kq) { return (kq ^ rg_key(row)) << 4; }
__device__ __forceinline__ int afrag_off(const int row, const int kq) { return row * 64 + afrag_slot(row, kq); }
// the RT row tiles (1 KB = 16 rows apart) x 2 planes of a step; base = the stage or image + this lane's afrag_off
template <int RT>
__device__ __forceinline__ void afrag_read(rg_u32x4 (&dst)[RT][2], const unsigned char* const base, const int plane_stride) {
#pragma unroll
  for (int mt = 0; mt < RT; ++mt)
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) dst[mt][pl] = *reinterpret_cast<const rg_u32x4*>(base + pl * plane_stride + mt * 1024);
}

}  // namespace jv
