// RoPE attention of the text encoder's layers in ONE launch (text_encoder.py:216-248, after the unchanged rope_qk pass):
//   att[i, h*288 ..] = softmax_j(q_i . k_j / sqrt(288)) V    over keys j < L_b, for queries i < L_b; rows L_b <= i < Tt are zeros
// with an online softmax over key tiles of 32: the [B, 2, Tt, Tt] score buffer of the four-launch route (encoder.hip
// enc_attention_gemm), which is what held jv_encoder_fwd to 512 tokens, never exists.
//
// Masked keys.  The reference, and the four-launch route, keep keys at and behind L_b in the softmax with masked_fill(-1e4).  For a
// valid query the row maximum is a real score, |score| <= |q| |k| / 17, and exp(-1e4 - max) underflows to exactly 0 in fp32 (and in
// fp64) unless max < -9900: the masked keys' probabilities are exactly 0 and their V rows never count.  Not reading them is therefore
// the same function, and a NaN there cannot meet a zero probability.  A padding query (i >= L_b) is different: all its scores are
// -1e4 there, the softmax is uniform and the row is an average of V that every consumer masks (conv_o is followed by
// layernorm_rows(..., mask)); here those rows are zeros.
//
// Arithmetic: every contraction is the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain), as relattn.hip
// and conv_gemm's fp32 route; exp is expf.  No operand is rounded to 16 bits.  Summation order: q . k is four chains of 72 terms
// summed pairwise, and a key tile's V^T P^T starts from zero and joins alpha O^T with one fma per element.  With one chain of 288
// and O accumulated key by key the error against fp64 grew to 1.1e-6 at 1025 tokens (q, k, v of order one); as written it stays
// below 8e-7 from 1 to 1025 tokens and below 3e-7 from 257 on (tests/test_gpu_encattn.py prints it).
//
// Geometry (relattn.hip's, for 2 heads of 288 columns).  A workgroup of two waves owns 64 queries of one (utterance, head); wave w
// owns queries I0 + 32 w .. + 31 as the MFMA's column index: every product is computed TRANSPOSED (S^T = K Q^T, O^T = V^T P^T), so a
// lane (i, g) -- i = lane & 31 its query, g = lane >> 5 -- holds, for its own query, 16 of a tile's 32 scores:
//   register r of lane (i, g)  <->  key  kap(r, g) = (r & 3) + 8 (r >> 2) + 4 g        (the 32x32 C/D map)
// The softmax is 16 registers and one exchange with lane i + 32, its rescale a per-lane scalar, and P^T is the B operand of the next
// product AS IT LIES: step k of O^T += V^T P^T contracts keys kap(k, 0) and kap(k, 1), and V^T is read from LDS in that order.
// q . k runs over d = 144 g + k, k = 0 .. 143 (a lane's half of its q row is contiguous in memory and lives in 144 registers);
// O^T of 32 queries x 288 columns is nine 32x32 accumulator tiles, 144 registers.  Together that is past 256: the kernel is built
// for ONE wave per SIMD (__launch_bounds__(128): two waves on a CU's four SIMDs), which gives the unified 512-register file.
//
// 64 queries per workgroup, not 128: a single long text has few (head, query-tile) workgroups -- Tt = 1024 gives 2 x 16 of them
// on 256 CUs -- and the 72 KiB of K/V tile let two workgroups share a CU.  32 queries (one wave) would double the workgroups again
// but leave every wave alone with its staging: nothing runs under a one-wave workgroup's global loads.
//
// The tile walk of utterance b is j0 = 0, 32, .. < L_b: it depends on L_b only, never on Tt or on batch neighbours, and an MFMA
// column (a query) never sees another column's operands, so an utterance's rows are bit-identical alone and in any batch.
//
// Not read: q rows at and behind L_b, k / v rows at and behind L_b (staged as zeros), rows of no utterance.  L_b = 0 reads nothing.
// Not written: rows of no utterance (guard rows and gaps).
#include <math.h>

#include "jv_model.h"

namespace jv {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int EA_D = 288;        // head columns
constexpr int EA_HALF = 144;     // a lane's half of the q . k contraction
constexpr int EA_NT = 9;         // 32-column output tiles
constexpr int EA_CH = 4;         // independent accumulators of q . k (36 MFMA steps of 2 columns each)
constexpr int EA_Q = 64;         // queries per workgroup (32 per wave)
constexpr int EA_K = 32;         // keys per tile
constexpr int EA_LDK = 289;      // K tile row stride (floats): lanes j = 0..31 of an A-operand read fall on 32 banks
constexpr int EA_LDV = 288;      // V tile: an A-operand read walks d, contiguous
constexpr int EA_SMEM = EA_K * EA_LDK + EA_K * EA_LDV;   // floats (72.1 KiB)
constexpr int EA_LDQ = 1728, EA_KOFF = 576, EA_VOFF = 1152, EA_LDO = 576;

__device__ __forceinline__ int kap(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

__global__ __launch_bounds__(128) void enc_attention_kernel(const float* __restrict__ qkv, const long* __restrict__ len, int T, int G,
                                                            int S, float* __restrict__ att) {
  extern __shared__ float smem[];
  float* const kt = smem;                                  // [32][289]  keys j0 .. j0 + 31, this head's 288 columns
  float* const vt = kt + EA_K * EA_LDK;                    // [32][288]

  const int b = blockIdx.z, hd = blockIdx.y, I0 = blockIdx.x * EA_Q;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
  const long lb = len[b];
  const int L = (int)(lb < 0 ? 0 : (lb > T ? T : lb));
  const long row0 = (long)G + (long)b * S;
  const int iq = I0 + 32 * wave + i;                       // this lane's query
  float* const orow = att + (row0 + iq) * EA_LDO + hd * EA_D;

  if (I0 >= L) {                                           // (uniform over the workgroup) nothing but padding rows here
    if (iq < T) {
#pragma unroll
      for (int c = 0; c < EA_HALF / 4; ++c) *reinterpret_cast<f32x4*>(orow + EA_HALF * g + 4 * c) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const bool qvalid = iq < L;
  const bool wave_on = I0 + 32 * wave < L;                 // (uniform over the wave)

  // this lane's q row, columns 144 g .. 144 g + 143 of the head
  float q[EA_HALF];
  {
    const float* qrow = qkv + (row0 + iq) * EA_LDQ + hd * EA_D + EA_HALF * g;
#pragma unroll
    for (int c = 0; c < EA_HALF / 4; ++c) {
      f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
      if (qvalid) q4 = *reinterpret_cast<const f32x4*>(qrow + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[4 * c + e] = q4[e];
    }
  }

  f32x16 o[EA_NT];                                         // O^T: tile t, register r = column 32 t + kap(r, g) of this lane's query
#pragma unroll
  for (int t = 0; t < EA_NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;
  const float inv = 1.0f / sqrtf(288.0f);

  for (int j0 = 0; j0 < L; j0 += EA_K) {
    // ---- stage K, V (zeros at and behind L) -------------------------------------------------------------------------------------
    __syncthreads();                                       // the previous tile's reads are done
    for (int idx = tid; idx < EA_K * (EA_D / 4); idx += 128) {
      const int r = idx / (EA_D / 4), c4 = idx - r * (EA_D / 4), j = j0 + r;
      f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = k4;
      if (j < L) {
        const float* src = qkv + (row0 + j) * EA_LDQ + hd * EA_D + 4 * c4;
        k4 = *reinterpret_cast<const f32x4*>(src + EA_KOFF);
        v4 = *reinterpret_cast<const f32x4*>(src + EA_VOFF);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) kt[r * EA_LDK + 4 * c4 + e] = k4[e];
      *reinterpret_cast<f32x4*>(vt + r * EA_LDV + 4 * c4) = v4;
    }
    __syncthreads();

    if (wave_on) {
      // ---- S^T = K Q^T ----------------------------------------------------------------------------------------------------------
      // (EA_CH independent fma chains of 72 terms, summed pairwise: a single chain of 288 is what the result's error hangs on)
      f32x16 sc[EA_CH];
#pragma unroll
      for (int c = 0; c < EA_CH; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[c][r] = 0.f;
      const float* ka = kt + i * EA_LDK + EA_HALF * g;
#pragma unroll
      for (int k = 0; k < EA_HALF / EA_CH; ++k)
#pragma unroll
        for (int c = 0; c < EA_CH; ++c) {
          const int kk = c * (EA_HALF / EA_CH) + k;
          sc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kk], q[kk], sc[c], 0, 0, 0);
        }
      f32x16 s = (sc[0] + sc[1]) + (sc[2] + sc[3]);
      // ---- scale, mask, online softmax -----------------------------------------------------------------------------------------
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = (qvalid && j0 + kap(r, g) < L) ? s[r] * inv : -INFINITY;
        tmax = fmaxf(tmax, s[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float mnew = fmaxf(mrun, tmax);
      float alpha = 1.f, psum = 0.f;
      if (mnew == -INFINITY) {                             // a padding query: nothing is ever seen
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
      } else {
        alpha = expf(mrun - mnew);                         // (mrun = -inf: 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = expf(s[r] - mnew);                        // (masked: exp(-inf) = 0)
          psum += s[r];
        }
      }
      psum += __shfl_xor(psum, 32);
      lrun = lrun * alpha + psum;
      mrun = mnew;
      // ---- O^T = alpha O^T + V^T P^T: step k contracts key kap(k, g) ------------------------------------------------------------
      // (the tile's product starts from zero and joins O once: a chain of 32 keys and one of L / 32 tiles, not one of L keys.
      // A 32x32x2 MFMA issues every 64 cycles and its result is ready after 64, so the dependent chain of a tile costs nothing)
#pragma unroll
      for (int t = 0; t < EA_NT; ++t) {
        f32x16 pv;
#pragma unroll
        for (int r = 0; r < 16; ++r) pv[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) pv = __builtin_amdgcn_mfma_f32_32x32x2f32(vt[kap(k, g) * EA_LDV + i + 32 * t], s[k], pv, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = fmaf(o[t][r], alpha, pv[r]);
      }
    }
  }

  if (iq < T) {
    const float rl = (qvalid && lrun > 0.f) ? 1.0f / lrun : 0.f;
#pragma unroll
    for (int t = 0; t < EA_NT; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {                        // registers 4 c .. 4 c + 3 are columns 32 t + 8 c + 4 g .. + 3
        f32x4 a = {o[t][4 * c], o[t][4 * c + 1], o[t][4 * c + 2], o[t][4 * c + 3]};
        if (!qvalid) a = f32x4{0.f, 0.f, 0.f, 0.f};        // (select: a padding query's accumulators are never multiplied out)
        *reinterpret_cast<f32x4*>(orow + 32 * t + 8 * c + 4 * g) = a * rl;
      }
  }
}

}  // namespace

int enc_attention(const float* qkv, const long* len, int B, int T, int G, int S, float* att, hipStream_t st) {
  if (B < 1 || T < 1) return JV_OK;
  if (S < T || G < 0) return fail(JV_ERR_ARG, "enc_attention: bad geometry");
  static bool inited = false;
  if (!inited) {
    JV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_attention_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               EA_SMEM * (int)sizeof(float)));
    inited = true;
  }
  prof_begin(st);
  hipLaunchKernelGGL(enc_attention_kernel, dim3(cdiv(T, EA_Q), 2, B), dim3(128), EA_SMEM * sizeof(float), st, qkv, len, T, G, S, att);
  JV_HIP(hipGetLastError());
  // 2 * 288 flops per (query, key) for each of q.k and P V
  prof_end(st, "enc_attention", 2.0 * B * 2.0 * 288.0 * 2.0 * (double)T * T, 4.0 * B * (double)T * (1728 + 576));
  return JV_OK;
}

}  // namespace jv
