// Relative-position attention of the UpsampleConformer blocks in ONE launch (attention.py:204-334, utils/mask.py:91-126,192-198):
//   s[i][j] = ((q_i + u_h) . k_j + (q_i + v_h) . p_h[T-1-i+j]) / 8   over keys j < lim(i) = min(L_b, (i / chunk + 1) * chunk),
//   att[i]  = softmax_j(s[i][:]) V,                                   rows L_b <= i < T written as zeros
// with an online softmax over key tiles of 32: neither ac = (q + u) K^T nor bd = (q + v) P^T (96 T^2 bytes per utterance and block on
// the three-GEMM route of prompt.hip) ever leaves the chip.  The token-to-mel route (flow_encoder_fwd) runs the encoder over whole
// utterances, where those buffers are what bounds the batch.
//
// Arithmetic: every contraction is the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain), as conv_gemm's
// fp32 route; exp is expf.  No operand is rounded to 16 bits.
//
// Geometry.  A workgroup of four waves owns 128 queries of one (utterance, head); wave w owns queries I0 + 32 w .. + 31 and keeps
// them as the MFMA's column index: every product is computed TRANSPOSED (S^T = K (Q+u)^T, O^T = V^T P^T), so that a lane (i, g) --
// i = lane & 31 its query, g = lane >> 5 -- holds, for its own query, 16 of a tile's 32 scores in its accumulator registers:
//   register r of lane (i, g)  <->  key  kap(r, g) = (r & 3) + 8 (r >> 2) + 4 g        (the 32x32 C/D map)
// The softmax of a query is then 16 registers and one exchange with lane i + 32, its rescale a per-lane scalar, and P^T is the B
// operand of the next product AS IT LIES: the k-th step of O^T += V^T P^T contracts key kap(k, g), the A operand V^T is read from LDS
// in that order.  A contraction's k order is free as long as both operands agree; q . k and q . p run over d = 32 g + k for the same
// reason (a lane's 32 q values are then contiguous in memory).
//
// Positional operand.  For the wave's 32 queries and a tile's 32 keys the rows of p that occur are T-1-i+j: ONE band of 63 rows,
// mw + (j - i + 31), mw = T - 1 - (I0 + 32 w) + j0 - 31.  The band product BD^T[m'][i] = p_h[mw + m'] . (q_i + v_h) is two MFMA tiles;
// it goes through a per-wave LDS image [i][m'] and comes back skewed, m' = kap(r, g) - i + 31, into the score registers.  The four
// waves' bands overlap: the workgroup stages the 160 rows T - I0 + j0 - 128 .. once per key tile.
//
// Not read: q rows at and behind L_b, k / v rows at and behind L_b (staged as zeros: a NaN there must not meet a zero
// probability), rows of p outside [0, 2T-1).  L_b = 0 reads nothing.
#include <math.h>

#include "jv_model.h"

namespace jv {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RA_Q = 128;        // queries per workgroup (32 per wave)
constexpr int RA_K = 32;         // keys per tile
constexpr int RA_LDK = 65;       // K tile row stride (floats): lanes j = 0..31 of an A-operand read fall on 32 banks
constexpr int RA_LDV = 64;       // V tile: an A-operand read walks d, contiguous
constexpr int RA_BAND = 160;     // band rows staged per tile: RA_Q + RA_K - 1 = 159, + 1 never-used row the second MFMA tile covers
constexpr int RA_LDB = 66;       // skew image row stride: the skewed read i * 66 + kap - i + 31 walks 65 i, one bank per lane
constexpr int RA_SMEM = RA_K * RA_LDK + RA_K * RA_LDV + RA_BAND * RA_LDK + 4 * 32 * RA_LDB;   // floats (92 KiB)

__device__ __forceinline__ int kap(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

__global__ __launch_bounds__(256) void rel_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ p, long p_rows,
                                                            const float* __restrict__ u, const float* __restrict__ v,
                                                            const long* __restrict__ len, int len_mul, int T, int G, int S, int chunk,
                                                            float* __restrict__ att) {
  extern __shared__ float smem[];
  float* const kt = smem;                                  // [32][65]  keys j0 .. j0 + 31, this head's 64 columns
  float* const vt = kt + RA_K * RA_LDK;                    // [32][64]
  float* const band = vt + RA_K * RA_LDV;                  // [160][65] rows m_lo .. m_lo + 159 of p, this head's 64 columns
  float* const skew = band + RA_BAND * RA_LDK;             // [4][32][66]

  const int b = blockIdx.z, hd = blockIdx.y, I0 = blockIdx.x * RA_Q;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
  const long lb = len[b] * (long)len_mul;
  const int L = (int)(lb < 0 ? 0 : (lb > T ? T : lb));
  const long row0 = (long)G + (long)b * S;
  const int iq = I0 + 32 * wave + i;                       // this lane's query
  float* const orow = att + (row0 + iq) * 512 + hd * 64;

  auto lim = [&](int q) { return chunk > 0 ? min(L, (q / chunk + 1) * chunk) : L; };   // keys query q < L may see

  if (I0 >= L) {                                           // (uniform over the workgroup) nothing but padding rows here
    if (iq < T) {
#pragma unroll
      for (int c = 0; c < 8; ++c) *reinterpret_cast<f32x4*>(orow + 32 * g + 4 * c) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const bool qvalid = iq < L;
  const int mylim = qvalid ? lim(iq) : 0;
  const bool wave_on = I0 + 32 * wave < L;                                  // (uniform over the wave)
  const int wave_lim = wave_on ? lim(min(I0 + 32 * wave + 31, L - 1)) : 0;   // lim is monotonic in the query
  const int blk_lim = lim(min(I0 + RA_Q - 1, L - 1));

  // this lane's q row, columns 32 g .. 32 g + 31 of the head, plus each bias
  float qu[32], qv[32];
  {
    const float* qrow = qkv + (row0 + iq) * 1536 + hd * 64 + 32 * g;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
      if (qvalid) q4 = *reinterpret_cast<const f32x4*>(qrow + 4 * c);
      const f32x4 u4 = *reinterpret_cast<const f32x4*>(u + hd * 64 + 32 * g + 4 * c);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(v + hd * 64 + 32 * g + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qu[4 * c + e] = q4[e] + u4[e];
        qv[4 * c + e] = q4[e] + v4[e];
      }
    }
  }

  f32x16 o0, o1;                                           // O^T: d = kap(r, g) and 32 + kap(r, g) of this lane's query
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;
  float* const myskew = skew + wave * 32 * RA_LDB;

  for (int j0 = 0; j0 < blk_lim; j0 += RA_K) {
    // ---- stage K, V (zeros at and behind L) and the band (zeros outside [0, p_rows)) -----------------------------------------
    __syncthreads();                                       // the previous tile's reads are done
    for (int idx = tid; idx < RA_K * 16; idx += 256) {
      const int r = idx >> 4, c4 = idx & 15, j = j0 + r;
      f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = k4;
      if (j < L) {
        const float* src = qkv + (row0 + j) * 1536 + hd * 64 + 4 * c4;
        k4 = *reinterpret_cast<const f32x4*>(src + 512);
        v4 = *reinterpret_cast<const f32x4*>(src + 1024);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) kt[r * RA_LDK + 4 * c4 + e] = k4[e];
      *reinterpret_cast<f32x4*>(vt + r * RA_LDV + 4 * c4) = v4;
    }
    const long m_lo = (long)T - I0 + j0 - RA_Q;
    for (int idx = tid; idx < RA_BAND * 16; idx += 256) {
      const int r = idx >> 4, c4 = idx & 15;
      const long m = m_lo + r;
      f32x4 p4 = {0.f, 0.f, 0.f, 0.f};
      if (m >= 0 && m < p_rows) p4 = *reinterpret_cast<const f32x4*>(p + m * 512 + hd * 64 + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) band[r * RA_LDK + 4 * c4 + e] = p4[e];
    }
    __syncthreads();

    const bool on = j0 < wave_lim;                         // (uniform over the wave) any of this wave's queries sees this tile
    f32x16 s;
    if (on) {
      // ---- S^T = K (Q + u)^T and the band product BD^T = P_band (Q + v)^T ---------------------------------------------------
      f32x16 bd0, bd1;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = bd0[r] = bd1[r] = 0.f;
      const float* ka = kt + i * RA_LDK + 32 * g;
      const float* ba = band + (96 - 32 * wave + i) * RA_LDK + 32 * g;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[k], qu[k], s, 0, 0, 0);
        bd0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ba[k], qv[k], bd0, 0, 0, 0);
        bd1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ba[32 * RA_LDK + k], qv[k], bd1, 0, 0, 0);
      }
      // BD^T[m'][i], m' = kap(r, g) (+ 32) -> skew image [i][m']
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        myskew[i * RA_LDB + kap(r, g)] = bd0[r];
        myskew[i * RA_LDB + 32 + kap(r, g)] = bd1[r];
      }
    }
    __syncthreads();
    if (on) {
      // ---- scores, mask, online softmax --------------------------------------------------------------------------------------
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = kap(r, g);
        const float sc = (s[r] + myskew[i * RA_LDB + jl - i + 31]) * 0.125f;
        s[r] = (j0 + jl < mylim) ? sc : -INFINITY;
        tmax = fmaxf(tmax, s[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float mnew = fmaxf(mrun, tmax);
      float alpha = 1.f, psum = 0.f;
      if (mnew == -INFINITY) {                             // nothing seen yet (a padding query, or a query whose keys start later)
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
      // ---- O^T = alpha O^T + V^T P^T: step k contracts key kap(k, g) --------------------------------------------------------
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[r] *= alpha;
        o1[r] *= alpha;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float* va = vt + kap(k, g) * RA_LDV + i;
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[0], s[k], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[32], s[k], o1, 0, 0, 0);
      }
    }
  }

  if (iq < T) {
    const float rl = (qvalid && lrun > 0.f) ? 1.0f / lrun : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                          // registers 4 c .. 4 c + 3 are d = 8 c + 4 g .. + 3
      f32x4 a = {o0[4 * c], o0[4 * c + 1], o0[4 * c + 2], o0[4 * c + 3]};
      f32x4 d = {o1[4 * c], o1[4 * c + 1], o1[4 * c + 2], o1[4 * c + 3]};
      if (!qvalid) a = d = f32x4{0.f, 0.f, 0.f, 0.f};      // (select: a padding query's accumulators are never multiplied out)
      *reinterpret_cast<f32x4*>(orow + 8 * c + 4 * g) = a * rl;
      *reinterpret_cast<f32x4*>(orow + 32 + 8 * c + 4 * g) = d * rl;
    }
  }
}

}  // namespace

int rel_attention(const float* qkv, const float* p, long p_rows, const float* u, const float* v, const long* len, int len_mul, int B,
                  int T, int G, int S, int chunk, float* att, hipStream_t st) {
  if (B < 1 || T < 1) return JV_OK;
  if (chunk < 0 || S < T || G < 0 || len_mul < 1) return fail(JV_ERR_ARG, "rel_attention: bad geometry or chunk");
  static bool inited = false;
  if (!inited) {
    JV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rel_attention_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               RA_SMEM * (int)sizeof(float)));
    inited = true;
  }
  prof_begin(st);
  hipLaunchKernelGGL(rel_attention_kernel, dim3(cdiv(T, RA_Q), 8, B), dim3(256), RA_SMEM * sizeof(float), st, qkv, p, p_rows, u, v,
                     len, len_mul, T, G, S, chunk, att);
  JV_HIP(hipGetLastError());
  // 2 * 64 flops per (query, key) for each of q.k, the 2x band of q.p, and P V
  prof_end(st, "rel_attention", 8.0 * B * 2.0 * 64.0 * 4.0 * (double)T * T, 4.0 * B * (double)T * (1536 + 512));
  return JV_OK;
}

}  // namespace jv
