// The no-gradient half of JyutVoiceTTS.forward (jyutvoice_tts.py:255-364): the log prior between text tokens and frames, the
// monotonic alignment search over it (utils/monotonic_align/core.pyx) and the pieces of the three losses.
//
//   log_prior   [b, x, y] = -0.5 sum_c (h[b, y, c] - mu_x[b, c, x])^2 - 0.5 log(2 pi) 80            jyutvoice_tts.py:306-314
//   search      core.pyx:19-37, in fp32, one workgroup per utterance                                 -> frame_index, attn, durations
//   losses      duration (utils/model.py:49-51), prior (jyutvoice_tts.py:349-362), flow matching (flow_matching.py:319-339)
//
// Prior.  The difference form, one fmaf per channel into four interleaved partial sums (c mod 4, each ascending), combined as
// (s0 + s1) + (s2 + s3): chains of 20 terms instead of one of 80, and an order that is a property of the kernel alone, so a cell
// has the same bits wherever its utterance lies in a batch.  A workgroup owns 16 frames x 64 tokens; h and mu_x tiles are
// staged in LDS SELECTING zero behind the lengths (nothing behind a length is read).  The result goes to a context buffer in
// [B, Ty, Tx] layout -- a column of the recurrence is then contiguous -- and, on request, to the caller in the reference's
// [B, Tx, Ty] layout with zeros outside x < x_len, y < y_len.
//
// Search.  Lanes own tokens x = tid + 256 k (k < NK; Tx <= 2048); the loop over frames y is sequential with the running column
// in LDS, double-buffered: column y reads buffer (y + 1) & 1 and writes buffer y & 1, then ONE __syncthreads().  Per column
//   cur  = (x == y) ? -1e9 : col[x]
//   prev = (x == 0) ? (y == 0 ? 0 : -1e9) : col[x - 1]
//   col'[x] = (prev > cur ? prev : cur) + log_prior[x, y]            for max(0, t_x + y - t_y) <= x < min(t_x, y + 1)
// -- one add, nothing to contract.  Cells of the band at column y read only cells of the band at column y - 1, so what lies
// outside the band is never read (and LDS is not initialised).  Beside the column one decision bit per cell, `cur < prev`
// (strict) on the values of column y - 1, a wave's 64 bits as one word of a context buffer [B, Ty, ceil(Tx / 64)].  The scores of
// the next CH columns are loaded while the current CH are computed: they do not depend on the recurrence.
// The backtrack (core.pyx:34-37) is wave 0's: 64 frames at a time, lane l loads the (at most two) words its frame can need --
// the index falls by at most one per frame -- and the wave walks them with shuffles, uniformly.  There is no waiting between
// workgroups anywhere: an utterance is one workgroup's work.  attn and durations are a second, wide launch over frame_index.
//
// Reductions (the losses, the durations) are per-workgroup partials in a fixed tree plus one finishing launch that adds the
// partials in a fixed order: no float atomics, run-to-run identical bits.
//
// The transposed prior, the decision bits, the partials and the pinned length vector belong to the context, grow on demand, are
// not workspace (jv_reserve leaves them alone) and are freed by jv_destroy.
#include <math.h>
#include <stdio.h>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"

namespace jv {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_NK = 8;                              // tokens per lane of the search: Tx <= 2048
constexpr int LP_TX = 64, LP_TY = 16;                     // the prior's tile
constexpr int GP_TY = 64;                                 // frames per workgroup of the gather / squared-error kernels
constexpr float AL_NEG = -1e9f;                           // core.pyx max_neg_val
constexpr float AL_LOG_2PI = 1.8378770664093453f;
constexpr float AL_PRIOR_CONST = -73.51508265637381f;     // -0.5 log(2 pi) 80
constexpr float AL_ONE_MINUS_SIGMA = 0.999999f;           // 1 - sigma_min (base.yaml sigma_min = 1e-6), as fp32

struct AlignWs {
  float* prior_t = nullptr;                 // [B][Ty][Tx]
  size_t prior_cap = 0;
  unsigned long long* bits = nullptr;       // [B][Ty][ceil(Tx / 64)]
  size_t bits_cap = 0;
  float* part = nullptr;                    // per-workgroup partials of the call in flight
  size_t part_cap = 0;
  int* h_lens = nullptr;                    // pinned: x_lens | y_lens of the call being validated
  size_t h_cap = 0;
};

void align_ws_destroy(Context& c) {
  if (!c.alws) return;
  (void)hipFree(c.alws->prior_t);
  (void)hipFree(c.alws->bits);
  (void)hipFree(c.alws->part);
  if (c.alws->h_lens) (void)hipHostFree(c.alws->h_lens);
  delete c.alws;
  c.alws = nullptr;
}

namespace {

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum over the workgroup in a fixed tree; the result is valid in thread 0
__device__ inline float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = AL_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// ---- log prior ------------------------------------------------------------------------------------------------------------
struct PriorArgs {
  const float* mu_x;      // [B, 80, Tx]
  const float* h;         // [B, Ty, 80]
  const int *x_lens, *y_lens;
  int Tx, Ty;
  float* prior_t;         // [B, Ty, Tx]
  float* out;             // [B, Tx, Ty] or null
};

__global__ __launch_bounds__(AL_THREADS) void log_prior_kernel(PriorArgs a) {
  __shared__ float mu_s[N_FEATS][LP_TX];
  __shared__ float h_s[LP_TY][N_FEATS];
  __shared__ float r_s[LP_TY][LP_TX + 1];
  const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * LP_TX, y0 = blockIdx.y * LP_TY;
  const int xl = clampi(a.x_lens[b], 0, a.Tx), yl = clampi(a.y_lens[b], 0, a.Ty);
  const int xx = tid & (LP_TX - 1), yg = tid >> 6;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (x0 < xl && y0 < yl) {      // (uniform) a tile wholly behind a length writes zeros and reads nothing
    for (int idx = tid; idx < N_FEATS * LP_TX; idx += AL_THREADS) {
      const int c = idx >> 6, x = x0 + (idx & (LP_TX - 1));
      mu_s[c][idx & (LP_TX - 1)] = x < xl ? a.mu_x[((long)b * N_FEATS + c) * a.Tx + x] : 0.f;
    }
    for (int idx = tid; idx < LP_TY * N_FEATS; idx += AL_THREADS) {
      const int yy = idx / N_FEATS, y = y0 + yy;
      h_s[yy][idx - yy * N_FEATS] = y < yl ? a.h[((long)b * a.Ty + y0) * N_FEATS + idx] : 0.f;
    }
    __syncthreads();
    float acc[4][4] = {};      // [frame][c mod 4]: four chains of 20 terms each, not one of 80
#pragma unroll 1      // (fully unrolled, the 80 channels' LDS loads are hoisted into 256 VGPRs + AGPRs: one wave per SIMD)
    for (int c = 0; c < N_FEATS; c += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float m = mu_s[c + q][xx];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = h_s[4 * yg + j][c + q] - m;
          acc[j][q] = fmaf(d, d, acc[j][q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sum = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
      v[j] = (x0 + xx < xl && y0 + 4 * yg + j < yl) ? fmaf(-0.5f, sum, AL_PRIOR_CONST) : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + 4 * yg + j;
    if (x0 + xx < a.Tx && y < a.Ty) a.prior_t[((long)b * a.Ty + y) * a.Tx + x0 + xx] = v[j];
    r_s[4 * yg + j][xx] = v[j];
  }
  if (!a.out) return;
  __syncthreads();
  for (int idx = tid; idx < LP_TX * LP_TY; idx += AL_THREADS) {
    const int x = idx >> 4, yy = idx & (LP_TY - 1);
    if (x0 + x < a.Tx && y0 + yy < a.Ty) a.out[((long)b * a.Tx + x0 + x) * a.Ty + y0 + yy] = r_s[yy][x];
  }
}

// [B, Tx, Ty] scores of the caller -> [B, Ty, Tx]; what lies behind the lengths is not read (it may be NaN)
__global__ __launch_bounds__(AL_THREADS) void score_transpose_kernel(const float* __restrict__ value, const int* __restrict__ x_lens,
                                                                     const int* __restrict__ y_lens, int Tx, int Ty,
                                                                     float* __restrict__ prior_t) {
  __shared__ float t[32][33];
  const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * 32, y0 = blockIdx.y * 32, tx = tid & 31, ty = tid >> 5;
  const int xl = clampi(x_lens[b], 0, Tx), yl = clampi(y_lens[b], 0, Ty);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + ty + 8 * j, y = y0 + tx;
    t[ty + 8 * j][tx] = (x < xl && y < yl) ? value[((long)b * Tx + x) * Ty + y] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + ty + 8 * j, x = x0 + tx;
    if (x < Tx && y < Ty) prior_t[((long)b * Ty + y) * Tx + x] = t[tx][ty + 8 * j];
  }
}

// ---- the search -------------------------------------------------------------------------------------------------------------
struct MasArgs {
  const float* prior_t;            // [B, Ty, Tx]
  const int *x_lens, *y_lens;
  int Tx, Ty, words;
  unsigned long long* bits;        // [B, Ty, words]
  int* frame_index;                // [B, Ty]
};

template <int NK>
__global__ __launch_bounds__(AL_THREADS) void mas_kernel(MasArgs a) {
  constexpr int CH = NK <= 2 ? 8 : 16 / NK;      // columns whose scores are in flight
  __shared__ float col[2][NK * AL_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int tx = a.x_lens[b], ty = a.y_lens[b];
  int* __restrict__ fi = a.frame_index + (long)b * a.Ty;
  if (tx < 1 || tx > a.Tx || ty < tx || ty > a.Ty) {      // rejected on the host before the launch; never trusted here
    for (int y = tid; y < a.Ty; y += AL_THREADS) fi[y] = -1;
    return;
  }
  const float* __restrict__ lp = a.prior_t + (long)b * a.Ty * a.Tx;
  unsigned long long* __restrict__ bits = a.bits + (long)b * a.Ty * a.words;
  for (int y = ty + tid; y < a.Ty; y += AL_THREADS) fi[y] = -1;

  float v[CH][NK], nv[CH][NK];
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int lo = max(0, tx + j - ty), hi = min(tx, j + 1);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int x = tid + AL_THREADS * k;
      v[j][k] = (j < ty && x >= lo && x < hi) ? lp[(long)j * a.Tx + x] : 0.f;
    }
  }
  for (int y0 = 0; y0 < ty; y0 += CH) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int y = y0 + CH + j, lo = max(0, tx + y - ty), hi = min(tx, y + 1);
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int x = tid + AL_THREADS * k;
        nv[j][k] = (y < ty && x >= lo && x < hi) ? lp[(long)y * a.Tx + x] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int y = y0 + j;
      if (y >= ty) break;      // (uniform)
      const float* cp = col[(y + 1) & 1];
      float* cn = col[y & 1];
      const int lo = max(0, tx + y - ty), hi = min(tx, y + 1);
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int x = tid + AL_THREADS * k;
        const bool in = x >= lo && x < hi;
        bool bit = false;
        if (in) {
          const float cur = x == y ? AL_NEG : cp[x];
          const float prev = x == 0 ? (y == 0 ? 0.f : AL_NEG) : cp[x - 1];
          cn[x] = (prev > cur ? prev : cur) + v[j][k];
          bit = cur < prev;
        }
        const unsigned long long word = __ballot(bit);
        if (lane == 0 && 4 * k + wave < a.words) bits[(long)y * a.words + 4 * k + wave] = word;
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
      for (int k = 0; k < NK; ++k) v[j][k] = nv[j][k];
  }
  __threadfence();
  __syncthreads();
  if (wave != 0) return;

  // the backtrack: frames yb, yb - 1, ... yb - 63 per round; lane l holds the words of frame yb - l
  int idx = tx - 1;
  for (int yb = ty - 1; yb >= 0; yb -= 64) {
    const int y = yb - lane, W = idx >> 6;
    unsigned long long hi = 0, lo = 0;
    if (y >= 0) {
      hi = bits[(long)y * a.words + W];
      if (W > 0) lo = bits[(long)y * a.words + W - 1];
    }
    int mine = -1;
    const int n = min(64, yb + 1);
    for (int l = 0; l < n; ++l) {
      const unsigned long long wh = __shfl(hi, l), wl = __shfl(lo, l);
      if (lane == l) mine = idx;
      const unsigned long long w = (idx >> 6) == W ? wh : wl;
      if (idx != 0 && (idx == yb - l || ((w >> (idx & 63)) & 1ull))) --idx;
    }
    if (y >= 0) fi[y] = mine;
  }
}

// attn [B, Tx, Ty] one-hot and durations [B, Tx] from frame_index: one wave per token row
__global__ __launch_bounds__(AL_THREADS) void mas_outputs_kernel(const int* __restrict__ frame_index, const int* __restrict__ x_lens,
                                                                 const int* __restrict__ y_lens, int Tx, int Ty, float* __restrict__ attn,
                                                                 int* __restrict__ durations) {
  const int lane = threadIdx.x & 63, x = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (x >= Tx) return;
  const int xl = clampi(x_lens[b], 0, Tx), yl = clampi(y_lens[b], 0, Ty);
  const int* __restrict__ fi = frame_index + (long)b * Ty;
  int cnt = 0;
  for (int y = lane; y < Ty; y += 64) {
    const bool hit = x < xl && y < yl && fi[y] == x;
    if (attn) attn[((long)b * Tx + x) * Ty + y] = hit ? 1.f : 0.f;
    cnt += hit ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0 && durations) durations[(long)b * Tx + x] = cnt;
}

// ---- loss pieces ------------------------------------------------------------------------------------------------------------
// part[b] = sum_{x < x_len} (logw - log(1e-8 + durations))^2      (utils/model.py:49-51, jyutvoice_tts.py:321; the duration
// predictor's logw is masked, so the reference's terms behind x_len are zeros: nothing behind the length is read)
__global__ __launch_bounds__(AL_THREADS) void dur_loss_kernel(const float* __restrict__ logw, const int* __restrict__ durations,
                                                              const int* __restrict__ x_lens, int Tx, float* __restrict__ part) {
  __shared__ float red[AL_THREADS];
  const int b = blockIdx.x, xl = clampi(x_lens[b], 0, Tx);
  float s = 0.f;
  for (int x = threadIdx.x; x < xl; x += AL_THREADS) {      // behind x_len the reference's term is its masked logw squared: 0
    const float e = logw[(long)b * Tx + x] - logf(1e-8f + (float)durations[(long)b * Tx + x]);
    s += e * e;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[b] = s;
}

// mu_y[b, :, y] = mu_x[b, :, frame_index[b, y]] (zeros behind y_len) and the tile's share of the prior loss
// sum 0.5 ((h - mu_y)^2 + log(2 pi)) y_mask (jyutvoice_tts.py:334-335, 357-361)
__global__ __launch_bounds__(AL_THREADS) void gather_prior_kernel(const float* __restrict__ mu_x, const float* __restrict__ h,
                                                                  const int* __restrict__ frame_index, const int* __restrict__ y_lens,
                                                                  int Tx, int Ty, float* __restrict__ mu_y, float* __restrict__ part) {
  __shared__ float h_s[GP_TY][N_FEATS + 1];
  __shared__ float red[AL_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, y0 = blockIdx.x * GP_TY;
  const int yl = clampi(y_lens[b], 0, Ty);
  for (int idx = tid; idx < GP_TY * N_FEATS; idx += AL_THREADS) {
    const int yy = idx / N_FEATS;
    h_s[yy][idx - yy * N_FEATS] = y0 + yy < yl ? h[((long)b * Ty + y0) * N_FEATS + idx] : 0.f;
  }
  __syncthreads();
  const int y = y0 + lane;
  const bool valid = y < yl;
  const int f = valid ? clampi(frame_index[(long)b * Ty + y], 0, Tx - 1) : 0;
  float s = 0.f;
  for (int c = wave; c < N_FEATS; c += 4) {
    const float m = valid ? mu_x[((long)b * N_FEATS + c) * Tx + f] : 0.f;
    if (y < Ty) mu_y[((long)b * N_FEATS + c) * Ty + y] = m;
    const float d = h_s[lane][c] - m;
    if (valid) s += 0.5f * (d * d + AL_LOG_2PI);
  }
  s = block_sum(s, red);
  if (tid == 0) part[(long)b * gridDim.x + blockIdx.x] = s;
}

// part[b, tile] = sum over the tile's frames y < len_b and all C channels of (p - q)^2
__global__ __launch_bounds__(AL_THREADS) void masked_sq_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                               const int* __restrict__ lens, int C, int T, float* __restrict__ part) {
  __shared__ float red[AL_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, y = blockIdx.x * GP_TY + lane;
  const bool valid = y < clampi(lens[b], 0, T);
  float s = 0.f;
  if (valid)
    for (int c = wave; c < C; c += 4) {
      const long i = ((long)b * C + c) * T + y;
      const float d = p[i] - q[i];
      s += d * d;
    }
  s = block_sum(s, red);
  if (tid == 0) part[(long)b * gridDim.x + blockIdx.x] = s;
}

// out[0] = (sum of n partials, fixed order) / (sum_b clamp(lens[b], 0, T) * chan)
__global__ __launch_bounds__(AL_THREADS) void loss_finish_kernel(const float* __restrict__ part, long n, const int* __restrict__ lens,
                                                                 int B, int T, float chan, float* __restrict__ out) {
  __shared__ float red[AL_THREADS];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += AL_THREADS) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    long den = 0;
    for (int b = 0; b < B; ++b) den += clampi(lens[b], 0, T);
    out[0] = s / ((float)den * chan);
  }
}

// the estimator's inputs of ConditionalCFM.compute_loss (flow_matching.py:319-334) and the condition prefix of
// jyutvoice_tts.py:325-330, in the reference's own order of roundings (no contraction)
struct CfmInArgs {
  const float *x1, *z, *t, *cfg, *mu_y, *spks;
  const int* cond_index;
  int B, T;
  float *y_t, *u, *mu_m, *spks_m, *cond;
};

__global__ __launch_bounds__(AL_THREADS) void cfm_inputs_kernel(CfmInArgs a) {
  const long n = (long)a.B * N_FEATS * a.T, idx = (long)blockIdx.x * AL_THREADS + threadIdx.x;
  if (idx < (long)a.B * N_FEATS) a.spks_m[idx] = __fmul_rn(a.spks[idx], a.cfg[idx / N_FEATS]);
  if (idx >= n) return;
  const int b = (int)(idx / ((long)N_FEATS * a.T)), y = (int)(idx % a.T);
  const float t = a.t[b], m = a.cfg[b], x1 = a.x1[idx], z = a.z[idx];
  const float w = __fsub_rn(1.f, __fmul_rn(t, AL_ONE_MINUS_SIGMA));
  a.y_t[idx] = __fadd_rn(__fmul_rn(w, z), __fmul_rn(t, x1));
  a.u[idx] = __fsub_rn(x1, __fmul_rn(AL_ONE_MINUS_SIGMA, z));
  a.mu_m[idx] = __fmul_rn(a.mu_y[idx], m);
  a.cond[idx] = y < a.cond_index[b] ? __fmul_rn(x1, m) : 0.f;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
AlignWs& get(Context& c) {
  if (!c.alws) c.alws = new AlignWs();
  return *c.alws;
}

template <class T>
int grow(T*& p, size_t& cap, size_t count) {
  if (count <= cap) return JV_OK;
  JV_HIP(hipDeviceSynchronize());      // a queued launch may still use the old one
  (void)hipFree(p);
  p = nullptr;
  cap = 0;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
  cap = count;
  return JV_OK;
}

// the shape against the context's capacities, then both length vectors with one synchronisation: 1 <= x_len <= Tx,
// x_len <= y_len <= Ty, else JV_ERR_ARG naming the utterance -- before anything is launched
int check_lengths(Context& c, const char* who, const int* x_lens, const int* y_lens, int B, int Tx, int Ty, hipStream_t st) {
  char msg[200];
  if (B < 1 || Tx < 1 || Ty < 1) return fail(JV_ERR_ARG, std::string(who) + ": B, Tx, Ty must be positive");
  if (!x_lens || !y_lens) return fail(JV_ERR_ARG, std::string(who) + ": null length vector");
  if (B > 65535) return fail(JV_ERR_SHAPE, std::string(who) + ": B beyond 65535");
  if (Tx > c.max_tokens || Ty > c.max_frames || Tx > AL_MAX_NK * AL_THREADS) {
    snprintf(msg, sizeof msg, "%s: Tx = %d, Ty = %d exceed the capacity given to jv_create (max_tokens %d, max_frames %d; Tx <= %d)", who,
             Tx, Ty, c.max_tokens, c.max_frames, AL_MAX_NK * AL_THREADS);
    return fail(JV_ERR_SHAPE, msg);
  }
  AlignWs& w = get(c);
  if ((size_t)2 * B > w.h_cap) {
    if (w.h_lens) (void)hipHostFree(w.h_lens);
    w.h_lens = nullptr;
    w.h_cap = 0;
    JV_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.h_lens), sizeof(int) * 2 * B));
    w.h_cap = (size_t)2 * B;
  }
  JV_HIP(hipMemcpyAsync(w.h_lens, x_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipMemcpyAsync(w.h_lens + B, y_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    const int x = w.h_lens[b], y = w.h_lens[B + b];
    if (x < 1 || x > Tx) {
      snprintf(msg, sizeof msg, "%s: utterance %d: %d tokens outside [1, Tx = %d]", who, b, x, Tx);
      return fail(JV_ERR_ARG, msg);
    }
    if (y < x || y > Ty) {
      snprintf(msg, sizeof msg, "%s: utterance %d: %d frames outside [tokens = %d, Ty = %d] (an alignment needs a frame per token)", who, b,
               y, x, Ty);
      return fail(JV_ERR_ARG, msg);
    }
  }
  return JV_OK;
}

int reserve(AlignWs& w, int B, int Tx, int Ty) {
  JV_TRY(grow(w.prior_t, w.prior_cap, (size_t)B * Ty * Tx));
  JV_TRY(grow(w.bits, w.bits_cap, (size_t)B * Ty * cdiv(Tx, 64)));
  return JV_OK;
}

void launch_prior(AlignWs& w, const float* mu_x, const float* h, const int* x_lens, const int* y_lens, int B, int Tx, int Ty, float* out,
                  hipStream_t st) {
  PriorArgs p;
  p.mu_x = mu_x; p.h = h; p.x_lens = x_lens; p.y_lens = y_lens; p.Tx = Tx; p.Ty = Ty; p.prior_t = w.prior_t; p.out = out;
  const bool prof = prof_on();
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(log_prior_kernel, dim3((unsigned)cdiv(Tx, LP_TX), (unsigned)cdiv(Ty, LP_TY), (unsigned)B), dim3(AL_THREADS), 0, st, p);
  if (prof) prof_end(st, "align_log_prior", 3.0 * B * (double)Tx * Ty * N_FEATS, 4.0 * B * ((double)Tx * Ty * (out ? 2 : 1) + 80.0 * (Tx + Ty)));
}

int launch_search(AlignWs& w, const int* x_lens, const int* y_lens, int B, int Tx, int Ty, float* attn, int* frame_index, int* durations,
                  hipStream_t st) {
  MasArgs m;
  m.prior_t = w.prior_t; m.x_lens = x_lens; m.y_lens = y_lens; m.Tx = Tx; m.Ty = Ty; m.words = cdiv(Tx, 64); m.bits = w.bits;
  m.frame_index = frame_index;
  const bool prof = prof_on();
  const int nk = cdiv(Tx, AL_THREADS);
  if (prof) prof_begin(st);
  if (nk <= 1) hipLaunchKernelGGL(mas_kernel<1>, dim3((unsigned)B), dim3(AL_THREADS), 0, st, m);
  else if (nk <= 2) hipLaunchKernelGGL(mas_kernel<2>, dim3((unsigned)B), dim3(AL_THREADS), 0, st, m);
  else if (nk <= 4) hipLaunchKernelGGL(mas_kernel<4>, dim3((unsigned)B), dim3(AL_THREADS), 0, st, m);
  else hipLaunchKernelGGL(mas_kernel<8>, dim3((unsigned)B), dim3(AL_THREADS), 0, st, m);
  if (prof) prof_end(st, "align_search", 2.0 * B * (double)Tx * Ty, 4.0 * B * (double)Tx * Ty);
  if (attn || durations) {
    if (prof) prof_begin(st);
    hipLaunchKernelGGL(mas_outputs_kernel, dim3((unsigned)cdiv(Tx, 4), (unsigned)B), dim3(AL_THREADS), 0, st, frame_index, x_lens, y_lens, Tx,
                       Ty, attn, durations);
    if (prof) prof_end(st, "align_outputs", 0.0, 4.0 * B * (double)Tx * Ty);
  }
  JV_HIP(hipGetLastError());
  return JV_OK;
}

}  // namespace

}  // namespace jv

#define AL_GUARD(ctx, who)                                                                                             \
  if (!(ctx)) return jv::fail(JV_ERR_ARG, who ": null context");                                                       \
  if ((ctx)->c.broken) return jv::fail(JV_ERR_STATE, who ": context unusable (jv_reserve); destroy it");               \
  JV_HIP(hipSetDevice((ctx)->c.device));

extern "C" {

int jv_log_prior(jv_context* ctx, const float* mu_x, const float* h, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty,
                 float* log_prior, void* stream) {
  AL_GUARD(ctx, "jv_log_prior");
  if (!mu_x || !h || !log_prior) return jv::fail(JV_ERR_ARG, "jv_log_prior: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  JV_TRY(jv::check_lengths(ctx->c, "jv_log_prior", x_lens, y_lens, B, Tx, Ty, st));
  jv::AlignWs& w = jv::get(ctx->c);
  JV_TRY(jv::reserve(w, B, Tx, Ty));
  jv::launch_prior(w, mu_x, h, x_lens, y_lens, B, Tx, Ty, log_prior, st);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int jv_maximum_path(jv_context* ctx, const float* value, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty, float* attn,
                    int32_t* frame_index, int32_t* durations, void* stream) {
  AL_GUARD(ctx, "jv_maximum_path");
  if (!value || !frame_index) return jv::fail(JV_ERR_ARG, "jv_maximum_path: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  JV_TRY(jv::check_lengths(ctx->c, "jv_maximum_path", x_lens, y_lens, B, Tx, Ty, st));
  jv::AlignWs& w = jv::get(ctx->c);
  JV_TRY(jv::reserve(w, B, Tx, Ty));
  hipLaunchKernelGGL(jv::score_transpose_kernel, dim3((unsigned)jv::cdiv(Tx, 32), (unsigned)jv::cdiv(Ty, 32), (unsigned)B),
                     dim3(jv::AL_THREADS), 0, st, value, x_lens, y_lens, Tx, Ty, w.prior_t);
  return jv::launch_search(w, x_lens, y_lens, B, Tx, Ty, attn, frame_index, durations, st);
}

int jv_align(jv_context* ctx, const float* mu_x, const float* h, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty,
             float* log_prior, float* attn, int32_t* frame_index, int32_t* durations, void* stream) {
  AL_GUARD(ctx, "jv_align");
  if (!mu_x || !h || !frame_index) return jv::fail(JV_ERR_ARG, "jv_align: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  JV_TRY(jv::check_lengths(ctx->c, "jv_align", x_lens, y_lens, B, Tx, Ty, st));
  jv::AlignWs& w = jv::get(ctx->c);
  JV_TRY(jv::reserve(w, B, Tx, Ty));
  jv::launch_prior(w, mu_x, h, x_lens, y_lens, B, Tx, Ty, log_prior, st);
  return jv::launch_search(w, x_lens, y_lens, B, Tx, Ty, attn, frame_index, durations, st);
}

int jv_align_losses(jv_context* ctx, const float* logw, const int32_t* durations, const int32_t* x_lens, const float* mu_x, const float* h,
                    const int32_t* frame_index, const int32_t* y_lens, int B, int Tx, int Ty, float* mu_y, float* dur_loss,
                    float* prior_loss, void* stream) {
  AL_GUARD(ctx, "jv_align_losses");
  if (!logw || !durations || !x_lens || !mu_x || !h || !frame_index || !y_lens || !mu_y || !dur_loss || !prior_loss)
    return jv::fail(JV_ERR_ARG, "jv_align_losses: null tensor");
  if (B < 1 || Tx < 1 || Ty < 1) return jv::fail(JV_ERR_ARG, "jv_align_losses: B, Tx, Ty must be positive");
  if (B > 65535) return jv::fail(JV_ERR_SHAPE, "jv_align_losses: B beyond 65535");
  hipStream_t st = static_cast<hipStream_t>(stream);
  jv::AlignWs& w = jv::get(ctx->c);
  const int tiles = jv::cdiv(Ty, jv::GP_TY);
  JV_TRY(jv::grow(w.part, w.part_cap, (size_t)B * (1 + tiles)));
  float* part_p = w.part + B;
  const bool prof = jv::prof_on();
  if (prof) jv::prof_begin(st);
  hipLaunchKernelGGL(jv::dur_loss_kernel, dim3((unsigned)B), dim3(jv::AL_THREADS), 0, st, logw, durations, x_lens, Tx, w.part);
  hipLaunchKernelGGL(jv::loss_finish_kernel, dim3(1), dim3(jv::AL_THREADS), 0, st, w.part, (long)B, x_lens, B, Tx, 1.f, dur_loss);
  hipLaunchKernelGGL(jv::gather_prior_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(jv::AL_THREADS), 0, st, mu_x, h, frame_index, y_lens,
                     Tx, Ty, mu_y, part_p);
  hipLaunchKernelGGL(jv::loss_finish_kernel, dim3(1), dim3(jv::AL_THREADS), 0, st, part_p, (long)B * tiles, y_lens, B, Ty,
                     (float)jv::N_FEATS, prior_loss);
  if (prof) jv::prof_end(st, "align_losses", 3.0 * B * (double)Ty * jv::N_FEATS, 12.0 * B * (double)Ty * jv::N_FEATS);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int jv_cfm_loss_inputs(jv_context* ctx, const float* x1, const float* z, const float* t, const float* cfg_mask, const int32_t* cond_index,
                       const float* mu_y, const float* spks, int B, int T, float* y_t, float* u, float* mu_masked, float* spks_masked,
                       float* cond, void* stream) {
  AL_GUARD(ctx, "jv_cfm_loss_inputs");
  if (!x1 || !z || !t || !cfg_mask || !cond_index || !mu_y || !spks || !y_t || !u || !mu_masked || !spks_masked || !cond)
    return jv::fail(JV_ERR_ARG, "jv_cfm_loss_inputs: null tensor");
  if (B < 1 || T < 1) return jv::fail(JV_ERR_ARG, "jv_cfm_loss_inputs: B, T must be positive");
  hipStream_t st = static_cast<hipStream_t>(stream);
  jv::CfmInArgs a;
  a.x1 = x1; a.z = z; a.t = t; a.cfg = cfg_mask; a.mu_y = mu_y; a.spks = spks; a.cond_index = cond_index; a.B = B; a.T = T;
  a.y_t = y_t; a.u = u; a.mu_m = mu_masked; a.spks_m = spks_masked; a.cond = cond;
  const long n = (long)B * jv::N_FEATS * T;
  if (jv::cdivl(n, jv::AL_THREADS) > (1L << 30)) return jv::fail(JV_ERR_SHAPE, "jv_cfm_loss_inputs: too many elements for one launch");
  const bool prof = jv::prof_on();
  if (prof) jv::prof_begin(st);
  hipLaunchKernelGGL(jv::cfm_inputs_kernel, dim3((unsigned)jv::cdivl(n, jv::AL_THREADS)), dim3(jv::AL_THREADS), 0, st, a);
  if (prof) jv::prof_end(st, "align_cfm_inputs", 8.0 * n, 28.0 * n);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int jv_masked_mse(jv_context* ctx, const float* a, const float* b, const int32_t* lens, int B, int C, int T, float* out, void* stream) {
  AL_GUARD(ctx, "jv_masked_mse");
  if (!a || !b || !lens || !out) return jv::fail(JV_ERR_ARG, "jv_masked_mse: null tensor");
  if (B < 1 || C < 1 || T < 1) return jv::fail(JV_ERR_ARG, "jv_masked_mse: B, C, T must be positive");
  hipStream_t st = static_cast<hipStream_t>(stream);
  jv::AlignWs& w = jv::get(ctx->c);
  const int tiles = jv::cdiv(T, jv::GP_TY);
  if (B > 65535) return jv::fail(JV_ERR_SHAPE, "jv_masked_mse: B beyond 65535");
  JV_TRY(jv::grow(w.part, w.part_cap, (size_t)B * tiles));
  const bool prof = jv::prof_on();
  if (prof) jv::prof_begin(st);
  hipLaunchKernelGGL(jv::masked_sq_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(jv::AL_THREADS), 0, st, a, b, lens, C, T, w.part);
  hipLaunchKernelGGL(jv::loss_finish_kernel, dim3(1), dim3(jv::AL_THREADS), 0, st, w.part, (long)B * tiles, lens, B, T, (float)C, out);
  if (prof) jv::prof_end(st, "align_masked_mse", 3.0 * B * (double)C * T, 8.0 * B * (double)C * T);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

}  // extern "C"
