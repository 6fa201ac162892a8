// The row tail of the row-owning kernels (rowgemm_kernel.h, rowconv_kernel.h, rowres_kernel.h, rowblock_kernel.h), in ONE place.
// Each of them ends by passing its accumulators through an LDS slab and reading them back as whole rows, a wave per row:
//   scale * colscale + bias (+ residual) -> max |value| into the utterance's slot -> two-pass LayerNorm over the row's 256
//   channels -> two fp16 planes.
// The project's bit-for-bit contracts between kernels (a shard equals the whole batch, split q|k|v equals the fused block,
// rowres equals two rowconv launches, a folded norm1 equals a stand-alone LayerNorm) hold because every kernel evaluates
// these expressions in the same association: they are written here once and the kernels call them.
// The pieces take and return VALUES (arrays by reference); loads, stores and the address of a tracking slot stay at the call
// site, in the place and order each kernel chose for them -- a helper that owns a store or a slot pointer moves the
// kernels' address arithmetic around (profiles/rowtail_isa.md has what was tried).  A wave holds whole rows: lane l has
// columns 4 l .. 4 l + 3 of each of its rows.
#pragma once
#include "jv_device.h"

namespace jv {

typedef _Float16 rg_f16x8 __attribute__((ext_vector_type(8)));
typedef float rg_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int rg_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int rg_u32x2 __attribute__((ext_vector_type(2)));

// ---- LayerNorm over the row's 256 channels, two-pass (as rowops.hip's layernorm256_kernel) ----
// sum[j] = the row's sum, sq[j] = the sum of squares of the centred row; N rows at a time so that their reductions overlap
template <int N>
__device__ __forceinline__ void ln256_moments(const rg_f32x4 (&v)[N], float (&sum)[N], float (&sq)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) sum[j] = wave_sum((v[j][0] + v[j][1]) + (v[j][2] + v[j][3]));
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const rg_f32x4 d = v[j] - sum[j] * (1.f / 256.f);
    sq[j] = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]));
  }
}
// 1 / sqrt(var + eps).  The kernels use it in two forms that give the same bits.  Per row, on the wave-uniform sq[j]; or for
// a group of rows in ONE evaluation (the correctly rounded division and square root are ~30 instructions; per row that was
// a third of rowblock_kernel's row pass): lane j takes row j's sq -- `var_l = lane == j ? sq[j] : var_l`, written out in the
// kernel: inside a helper that select kept sq[] in scratch -- evaluates this once, and lane_bcast(result, j) is row j's.
__device__ __forceinline__ float ln256_rstd(const float sq, const float eps) { return 1.0f / sqrtf(sq * (1.f / 256.f) + eps); }
__device__ __forceinline__ float lane_bcast(const float v, const int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}
__device__ __forceinline__ rg_f32x4 ln256_apply(const rg_f32x4 v, const float sum, const float rstd, const rg_f32x4 g, const rg_f32x4 b) {
  const float mean = sum * (1.f / 256.f);
  return (v - mean) * rstd * g + b;
}

// ---- four columns -> their words of the two fp16 planes (value ~= h + l: split2h_pair); the caller stores them ----
struct Planes4 { rg_u32x2 h, l; };
__device__ __forceinline__ Planes4 split2h_x4(const rg_f32x4 y) {
  const Split2 s0 = split2h_pair(y[0], y[1]);
  const Split2 s1 = split2h_pair(y[2], y[3]);
  return {rg_u32x2{s0.h, s1.h}, rg_u32x2{s0.l, s1.l}};
}
__device__ __forceinline__ Planes4 split2h_x4(const rg_f32x4 y, const float scale) {
  const Split2 s0 = split2h_pair(y[0] * scale, y[1] * scale);
  const Split2 s1 = split2h_pair(y[2] * scale, y[3] * scale);
  return {rg_u32x2{s0.h, s1.h}, rg_u32x2{s0.l, s1.l}};
}

// ---- measured-bound tracking: max |value| of a row into its utterance's slot (the integer max of the bit patterns) ----
//   unsigned u = absmax4(v);
//   if (absmax_exceeds(tracked, u, seen)) {      // wave-uniform
//     u = wave_umax(u);
//     if (lane == 0) atomicMax(<the slot>, u);   // the slot's address is the caller's: computed where it computes it today
//   }
// `seen` is the slot's value as read earlier by a plain, cacheable load: the slot only grows, so a stale value is a valid
// lower bound and there is nothing to do once it holds a larger value than every lane's.
__device__ __forceinline__ unsigned absmax4(const rg_f32x4 v) {
  unsigned u = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) u = max(u, __float_as_uint(v[e]) & 0x7fffffffu);
  return u;
}
__device__ __forceinline__ bool absmax_exceeds(const bool tracked, const unsigned u, const unsigned seen) {
  return tracked && __builtin_amdgcn_ballot_w64(u > seen) != 0;
}
__device__ __forceinline__ unsigned wave_umax(unsigned u) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, o));
  return u;
}

}  // namespace jv
