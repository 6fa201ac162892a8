// Levels on the GPU: the energy trim of a voice prompt (librosa.effects.trim's contract), the sample peak, the integrated
// loudness of ITU-R BS.1770-4 (mono) and the gain that follows from them, for a ragged batch with device lengths in and out.
// All four are restated in include/jyutvoice_hip.h (unpinned: librosa and pyloudnorm are not part of this build).
//
// Trim.  A wave owns one frame: lane l adds x^2 at i = l, l + 64, ... < F in ascending i (one fmaf chain per lane), the 64
// partial sums meet in a fixed xor butterfly, so a frame's mean square does not depend on where the frame lies in a batch.  The
// maximum over a recording's frames is an integer atomic max on the bit pattern of a non-negative float (order-independent),
// the first / last non-silent frame an integer atomic min / max.
//
// Loudness.  K-weighting is two biquads in cascade, a linear recurrence with a 4-vector state z (transposed direct form II):
//   z' = A z + c x.  A recording is cut into segments of LV_SEG samples, one per lane:
//   1. loud_scan: lane l of a wave filters its segment from zero state (end state e_l).  The wave's 64 x LV_SEG samples are
//      staged through LDS (coalesced global reads; rows padded to LV_SEG + 1 words, so lane l reading word j of its row touches
//      bank (l + j) mod 32: conflict-free by the bank rule).  A Kogge-Stone scan over the wave with the host's table
//      P[d] = A^(LV_SEG d) turns e_l into the state each segment would start from had the WAVE started from zero.
//   2. loud_carry: one wave per recording scans the waves' end states the same way with Q[d] = A^(64 LV_SEG d), 64 waves per
//      round, carrying across rounds: every wave's true start state.
//   3. loud_bins: lane l starts from (its state from 1) + P[l] (its wave's start state from 2), filters its segment again and
//      adds y^2 into the 100 ms bin the sample falls into -- a segment meets at most one bin boundary (LV_SEG <= h), so two sums
//      per segment.
//   4. loud_gate: one wave per recording adds each bin from its segments in ascending order, forms z_j from four consecutive
//      bins, applies both gates in the linear domain and writes L.
// The recurrence, the carries and every sum run in fp64 (the coefficients are evaluated in fp64 on the host; x is exact in
// fp64): the high-pass has its poles 5e-3 from the unit circle and the carry is exact up to fp64 rounding, so nothing is
// truncated -- the distance to the fp64 definition is the final rounding of L to fp32.  Every order above is fixed by the
// sample index alone: a recording gives the same bits alone and in any ragged batch.
#include <math.h>
#include <stdio.h>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"

namespace jv {

constexpr int LV_THREADS = 256;
constexpr int LV_SEG = 32;                       // samples per lane
constexpr int LV_ROW = LV_SEG + 1;               // LDS row pitch in words
constexpr int LV_WSPAN = 64 * LV_SEG;            // samples per wave
constexpr int LV_GSPAN = 4 * LV_WSPAN;           // samples per workgroup
constexpr int LV_TILE = 4096;                    // samples per workgroup of the peak / apply kernels
constexpr int LV_TAB = 65 * 16;                  // doubles of one power table (d = 0 .. 64, 4 x 4 each)
constexpr int LV_CACHE = 8;                      // sample rates kept per context
constexpr long LV_MAX_GROUPS = 1L << 24;
constexpr int LV_MAX_FRAME = 8192;

struct KWeight { double sb0, sb1, sb2, sa1, sa2, hb0, hb1, hb2, ha1, ha2; };

struct LevelTab {
  int fs = 0;
  double* dev = nullptr;     // P[65][16] then Q[65][16]
  unsigned long used = 0;
};

struct LevelWs {
  std::vector<LevelTab> tabs;
  unsigned long clock = 0;
  void* scratch = nullptr;   // per-call intermediates of jv_trim_bounds / jv_loudness
  size_t scratch_bytes = 0;
};

void level_ws_destroy(Context& c) {
  if (!c.lws) return;
  for (LevelTab& t : c.lws->tabs) (void)hipFree(t.dev);
  (void)hipFree(c.lws->scratch);
  delete c.lws;
  c.lws = nullptr;
}

namespace {

KWeight kweight(int fs) {
  KWeight k;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / (double)fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    k.sb0 = (Vh + Vb * K / Q + K * K) / a0;
    k.sb1 = 2.0 * (K * K - Vh) / a0;
    k.sb2 = (Vh - Vb * K / Q + K * K) / a0;
    k.sa1 = 2.0 * (K * K - 1.0) / a0;
    k.sa2 = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / (double)fs), a0 = 1.0 + K / Q + K * K;
    k.hb0 = 1.0; k.hb1 = -2.0; k.hb2 = 1.0;
    k.ha1 = 2.0 * (K * K - 1.0) / a0;
    k.ha2 = (1.0 - K / Q + K * K) / a0;
  }
  return k;
}

bool rate_ok(int fs) { return fs >= 8000 && fs <= 192000; }
inline int block_hop(int fs) { return (fs + 5) / 10; }

typedef long double Mat4[4][4];

void mat_mul(const Mat4 a, const Mat4 b, Mat4 out) {
  Mat4 t;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      long double s = 0;
      for (int k = 0; k < 4; ++k) s += a[i][k] * b[k][j];
      t[i][j] = s;
    }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out[i][j] = t[i][j];
}

// tab[d] = base^d, d = 0 .. 64, row-major 4 x 4
void power_table(const Mat4 base, double* tab) {
  Mat4 cur = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int d = 0; d <= 64; ++d) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) tab[d * 16 + i * 4 + j] = (double)cur[i][j];
    mat_mul(base, cur, cur);
  }
}

// P[d] = A^(LV_SEG d) and Q[d] = A^(64 LV_SEG d), A the zero-input transition of kw_step below
void level_tables(const KWeight& k, double* tab) {
  const long double sa1 = k.sa1, sa2 = k.sa2, ha1 = k.ha1, ha2 = k.ha2, hb0 = k.hb0, hb1 = k.hb1, hb2 = k.hb2;
  Mat4 A = {{-sa1, 1, 0, 0}, {-sa2, 0, 0, 0}, {hb1 - ha1 * hb0, 0, -ha1, 1}, {hb2 - ha2 * hb0, 0, -ha2, 0}};
  Mat4 As = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int i = 0; i < LV_SEG; ++i) mat_mul(A, As, As);
  power_table(As, tab);
  Mat4 Aw;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) Aw[i][j] = As[i][j];
  for (int i = 0; i < 6; ++i) mat_mul(Aw, Aw, Aw);      // (A^LV_SEG)^64
  power_table(Aw, tab + LV_TAB);
}

struct V4 { double a, b, c, d; };

// one sample through shelf then high-pass (transposed direct form II); returns y
__device__ __forceinline__ double kw_step(const KWeight& k, V4& z, double x) {
  const double y1 = fma(k.sb0, x, z.a);
  z.a = fma(k.sb1, x, fma(-k.sa1, y1, z.b));
  z.b = fma(k.sb2, x, -k.sa2 * y1);
  const double y = fma(k.hb0, y1, z.c);
  z.c = fma(k.hb1, y1, fma(-k.ha1, y, z.d));
  z.d = fma(k.hb2, y1, -k.ha2 * y);
  return y;
}

// v + M u, M row-major 4 x 4
__device__ __forceinline__ V4 mat_acc(const double* __restrict__ M, const V4& u, V4 v) {
  v.a = fma(M[3], u.d, fma(M[2], u.c, fma(M[1], u.b, fma(M[0], u.a, v.a))));
  v.b = fma(M[7], u.d, fma(M[6], u.c, fma(M[5], u.b, fma(M[4], u.a, v.b))));
  v.c = fma(M[11], u.d, fma(M[10], u.c, fma(M[9], u.b, fma(M[8], u.a, v.c))));
  v.d = fma(M[15], u.d, fma(M[14], u.c, fma(M[13], u.b, fma(M[12], u.a, v.d))));
  return v;
}

__device__ __forceinline__ V4 shfl_up4(const V4& v, int d) {
  V4 u;
  u.a = __shfl_up(v.a, d); u.b = __shfl_up(v.b, d); u.c = __shfl_up(v.c, d); u.d = __shfl_up(v.d, d);
  return u;
}

// inclusive scan over the 64 lanes: v_l <- sum_{j <= l} tab[l - j] v_j (tab[d] = the transition over d lanes' spans)
__device__ __forceinline__ V4 wave_scan(V4 v, const double* __restrict__ tab, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V4 u = shfl_up4(v, d);
    if (lane >= d) v = mat_acc(tab + d * 16, u, v);
  }
  return v;
}

struct LoudArgs {
  const float* wav;
  const int* lens;
  int n, h, groups;          // row length, samples per 100 ms bin, workgroups per recording
  KWeight k;
  const double* tab;         // P then Q
  double* seg;               // [B][groups * 256][4]  a segment's start state had its wave started from zero
  double* sums;              // [B][groups * 256][2]  its y^2 before / behind the bin boundary it meets
  double* wend;              // [B][groups * 4][4]    a wave's end state from zero
  double* wst;               // [B][groups * 4][4]    a wave's true start state
  double* bins;              // [B][nbin]
  long nbin;
  double abs_thr;         // 10^((-70 + 0.691) / 10): the absolute gate on z
  float* lufs;
};

__device__ __forceinline__ void stage_wave(const float* __restrict__ x, long wbase, int len, int lane, float* tile) {
#pragma unroll 4
  for (int it = 0; it < LV_SEG; ++it) {
    const int i = it * 64 + lane;
    const long g = wbase + i;
    tile[(i / LV_SEG) * LV_ROW + (i % LV_SEG)] = g < len ? x[g] : 0.f;
  }
}

__global__ __launch_bounds__(LV_THREADS) void loud_scan_kernel(LoudArgs a) {
  __shared__ float lds[4 * 64 * LV_ROW];
  const int b = (int)(blockIdx.x / (unsigned)a.groups), g = (int)(blockIdx.x - (unsigned)b * (unsigned)a.groups);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const long base = (long)g * LV_GSPAN;
  if (base >= len) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* tile = lds + wave * 64 * LV_ROW;
  stage_wave(a.wav + (long)b * a.n, base + (long)wave * LV_WSPAN, len, lane, tile);
  __syncthreads();
  V4 z = {0.0, 0.0, 0.0, 0.0};
  const float* row = tile + lane * LV_ROW;
#pragma unroll 4
  for (int j = 0; j < LV_SEG; ++j) (void)kw_step(a.k, z, (double)row[j]);
  const V4 incl = wave_scan(z, a.tab, lane);
  V4 excl = shfl_up4(incl, 1);
  if (lane == 0) excl = V4{0.0, 0.0, 0.0, 0.0};
  const long s = ((long)b * a.groups + g) * LV_THREADS + threadIdx.x;
  a.seg[s * 4 + 0] = excl.a; a.seg[s * 4 + 1] = excl.b; a.seg[s * 4 + 2] = excl.c; a.seg[s * 4 + 3] = excl.d;
  if (lane == 63) {
    const long w = ((long)b * a.groups + g) * 4 + wave;
    a.wend[w * 4 + 0] = incl.a; a.wend[w * 4 + 1] = incl.b; a.wend[w * 4 + 2] = incl.c; a.wend[w * 4 + 3] = incl.d;
  }
}

// one wave per recording: the true start state of each of its waves
__global__ __launch_bounds__(64) void loud_carry_kernel(LoudArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const long nw = ((long)len + LV_WSPAN - 1) / LV_WSPAN;      // all of them lie in workgroups loud_scan_kernel ran
  const double* __restrict__ Q = a.tab + LV_TAB;
  const double* __restrict__ we = a.wend + (long)b * a.groups * 16;
  double* __restrict__ ws = a.wst + (long)b * a.groups * 16;
  V4 carry = {0.0, 0.0, 0.0, 0.0};
  for (long w0 = 0; w0 < nw; w0 += 64) {
    const long w = w0 + lane;
    V4 e = {0.0, 0.0, 0.0, 0.0};
    if (w < nw) e = V4{we[w * 4], we[w * 4 + 1], we[w * 4 + 2], we[w * 4 + 3]};
    V4 incl = wave_scan(e, Q, lane);
    incl = mat_acc(Q + (lane + 1) * 16, carry, incl);
    V4 excl = shfl_up4(incl, 1);
    if (lane == 0) excl = carry;
    if (w < nw) { ws[w * 4] = excl.a; ws[w * 4 + 1] = excl.b; ws[w * 4 + 2] = excl.c; ws[w * 4 + 3] = excl.d; }
    carry.a = __shfl(incl.a, 63); carry.b = __shfl(incl.b, 63); carry.c = __shfl(incl.c, 63); carry.d = __shfl(incl.d, 63);
  }
}

__global__ __launch_bounds__(LV_THREADS) void loud_bins_kernel(LoudArgs a) {
  __shared__ float lds[4 * 64 * LV_ROW];
  const int b = (int)(blockIdx.x / (unsigned)a.groups), g = (int)(blockIdx.x - (unsigned)b * (unsigned)a.groups);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const long base = (long)g * LV_GSPAN;
  if (base >= len) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* tile = lds + wave * 64 * LV_ROW;
  const long wbase = base + (long)wave * LV_WSPAN;
  stage_wave(a.wav + (long)b * a.n, wbase, len, lane, tile);
  __syncthreads();
  const long s = ((long)b * a.groups + g) * LV_THREADS + threadIdx.x;
  const long w = ((long)b * a.groups + g) * 4 + wave;
  // a wave behind the recording's end has no start state (loud_carry_kernel stops at the last wave with samples) and no bin
  V4 z = {0.0, 0.0, 0.0, 0.0};
  if (wbase < len) {
    const V4 s0 = {a.wst[w * 4], a.wst[w * 4 + 1], a.wst[w * 4 + 2], a.wst[w * 4 + 3]};
    z = mat_acc(a.tab + lane * 16, s0, V4{a.seg[s * 4], a.seg[s * 4 + 1], a.seg[s * 4 + 2], a.seg[s * 4 + 3]});
  }
  const long i0 = wbase + (long)lane * LV_SEG;
  const long bnd = (i0 / a.h + 1) * a.h;      // the one bin boundary the segment can meet
  const float* row = tile + lane * LV_ROW;
  double before = 0.0, behind = 0.0;
#pragma unroll 4
  for (int j = 0; j < LV_SEG; ++j) {
    const double y = kw_step(a.k, z, (double)row[j]);
    if (i0 + j < bnd) before = fma(y, y, before);
    else behind = fma(y, y, behind);
  }
  a.sums[s * 2] = before;
  a.sums[s * 2 + 1] = behind;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// one wave per recording: bins from segments in ascending order, blocks of four bins, both gates, L
__global__ __launch_bounds__(64) void loud_gate_kernel(LoudArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const long nfull = len / a.h;      // complete bins: all their segments lie in workgroups loud_bins_kernel ran
  const double* __restrict__ sums = a.sums + (long)b * a.groups * LV_THREADS * 2;
  double* __restrict__ bins = a.bins + (long)b * a.nbin;
  for (long j = lane; j < nfull; j += 64) {
    const long k0 = j * a.h / LV_SEG, k1 = ((j + 1) * a.h - 1) / LV_SEG;
    double acc = 0.0;
    for (long k = k0; k <= k1; ++k) acc += (k * LV_SEG / a.h == j) ? sums[k * 2] : sums[k * 2 + 1];
    bins[j] = acc;
  }
  __syncthreads();
  const long nb = nfull >= 4 ? nfull - 3 : 0;
  const double inv = 1.0 / (4.0 * (double)a.h);
  const double abs_thr = a.abs_thr;
  double s1 = 0.0, c1 = 0.0;
  for (long j = lane; j < nb; j += 64) {
    const double z = (((bins[j] + bins[j + 1]) + bins[j + 2]) + bins[j + 3]) * inv;
    if (z > abs_thr) { s1 += z; c1 += 1.0; }
  }
  s1 = wave_sum(s1);
  c1 = wave_sum(c1);
  float L = -INFINITY;
  if (c1 > 0.0) {
    const double rel_thr = 0.1 * (s1 / c1);
    double s2 = 0.0, c2 = 0.0;
    for (long j = lane; j < nb; j += 64) {
      const double z = (((bins[j] + bins[j + 1]) + bins[j + 2]) + bins[j + 3]) * inv;
      if (z > abs_thr && z > rel_thr) { s2 += z; c2 += 1.0; }
    }
    s2 = wave_sum(s2);
    c2 = wave_sum(c2);
    if (c2 > 0.0) L = (float)(-0.691 + 10.0 * log10(s2 / c2));
  }
  if (lane == 0) a.lufs[b] = L;
}

// ---- trim -------------------------------------------------------------------------------------------------------
struct TrimArgs {
  const float* wav;
  const int* lens;
  int n, F, H, Tmax, tiles;      // tiles: workgroups per recording (4 frames each)
  float thr;                     // 10^(-top_db / 10)
  float* ms;                     // [B][Tmax] max(1e-10, mean square)
  unsigned* mx;                  // [B] bits of the recording's maximum
  int* first;                    // [B] first / last non-silent frame
  int* last;
  int* start;
  int* end;
};

__device__ __forceinline__ int trim_frames(int len, int F, int H) {
  const long span = (long)len + 2 * (F / 2) - F;
  return (len == 0 || span < 0) ? 0 : (int)(1 + span / H);
}

__global__ void trim_init_kernel(TrimArgs a, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  a.mx[b] = 0u;
  a.first[b] = 0x7fffffff;
  a.last[b] = -1;
}

__global__ __launch_bounds__(LV_THREADS) void trim_energy_kernel(TrimArgs a) {
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const int t = tile * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= trim_frames(len, a.F, a.H)) return;
  const float* __restrict__ x = a.wav + (long)b * a.n;
  const long i0 = (long)t * a.H - a.F / 2;
  float acc = 0.f;
  for (int i = lane; i < a.F; i += 64) {
    const long g = i0 + i;
    const float v = (g >= 0 && g < len) ? x[g] : 0.f;
    acc = fmaf(v, v, acc);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  const float m = fmaxf(1e-10f, acc / (float)a.F);
  if (lane == 0) {
    a.ms[(long)b * a.Tmax + t] = m;
    atomicMax(a.mx + b, __float_as_uint(m));
  }
}

__global__ __launch_bounds__(LV_THREADS) void trim_mark_kernel(TrimArgs a, int per) {
  const int b = (int)(blockIdx.x / (unsigned)per), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)per);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const int t = tile * LV_THREADS + threadIdx.x;
  if (t >= trim_frames(len, a.F, a.H)) return;
  const float M = __uint_as_float(a.mx[b]);
  if (a.ms[(long)b * a.Tmax + t] > M * a.thr) {
    atomicMin(a.first + b, t);
    atomicMax(a.last + b, t);
  }
}

__global__ void trim_finish_kernel(TrimArgs a, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const int last = a.last[b];
  a.start[b] = last < 0 ? 0 : (int)min((long)len, (long)a.first[b] * a.H);
  a.end[b] = last < 0 ? 0 : (int)min((long)len, ((long)last + 1) * a.H);
}

// ---- peak, gain, apply -------------------------------------------------------------------------------------------
__device__ __forceinline__ void level_range(const int* lens, const int* start, const int* end, int b, int n, int& s, int& e) {
  const int len = lens ? min(max(lens[b], 0), n) : n;
  s = start ? min(max(start[b], 0), len) : 0;
  e = end ? min(max(end[b], s), len) : len;
}

__global__ __launch_bounds__(LV_THREADS) void peak_kernel(const float* __restrict__ wav, const int* __restrict__ lens,
                                                          const int* __restrict__ start, const int* __restrict__ end, int n, int tiles,
                                                          unsigned* __restrict__ peak) {
  const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
  int s, e;
  level_range(lens, start, end, b, n, s, e);
  const long j0 = (long)s + (long)tile * LV_TILE, j1 = min(j0 + LV_TILE, (long)e);
  float m = 0.f;
  for (long j = j0 + threadIdx.x; j < j1; j += LV_THREADS) m = fmaxf(m, fabsf(wav[(long)b * n + j]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(peak + b, __float_as_uint(m));
}

__global__ void gain_kernel(const float* __restrict__ lufs, const float* __restrict__ peak, int B, double target, double ceiling,
                            float* __restrict__ gain) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float p = peak ? peak[b] : 0.f;
  double g = 1.0;
  if (!lufs) {      // the prompt rule: down to the ceiling, never up
    if ((double)p > ceiling) g = ceiling / (double)p;
  } else {
    const float L = lufs[b];
    if (L > -INFINITY && !(peak && p == 0.f)) {
      g = pow(10.0, (target - (double)L) / 20.0);
      if (peak && ceiling > 0.0) g = fmin(g, ceiling / (double)p);
    }
  }
  gain[b] = (float)g;
}

__global__ __launch_bounds__(LV_THREADS) void apply_kernel(const float* __restrict__ wav, const int* __restrict__ lens,
                                                           const int* __restrict__ start, const int* __restrict__ end,
                                                           const float* __restrict__ gain, int n, int tail, float* __restrict__ out,
                                                           long n_out, int* __restrict__ out_lens, int tiles) {
  const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
  int s, e;
  level_range(lens, start, end, b, n, s, e);
  if (tile == 0 && threadIdx.x == 0 && out_lens) out_lens[b] = e - s + tail;
  const float g = gain ? gain[b] : 1.f;
  const float* __restrict__ x = wav + (long)b * n + s;
  const long j0 = (long)tile * LV_TILE, j1 = min(j0 + LV_TILE, n_out), keep = e - s;
  for (long j = j0 + threadIdx.x; j < j1; j += LV_THREADS) out[(long)b * n_out + j] = j < keep ? x[j] * g : 0.f;
}

LevelWs& get(Context& c) {
  if (!c.lws) c.lws = new LevelWs();
  return *c.lws;
}

int scratch_reserve(LevelWs& w, size_t bytes) {
  if (bytes <= w.scratch_bytes) return JV_OK;
  JV_HIP(hipDeviceSynchronize());      // a queued launch may still use the old one
  (void)hipFree(w.scratch);
  w.scratch = nullptr;
  w.scratch_bytes = 0;
  JV_HIP(hipMalloc(&w.scratch, bytes));
  w.scratch_bytes = bytes;
  return JV_OK;
}

// the cached power tables of a sample rate, built and uploaded on a miss
int level_table(LevelWs& w, int fs, const KWeight& k, const double** dev) {
  ++w.clock;
  for (LevelTab& t : w.tabs)
    if (t.fs == fs) {
      t.used = w.clock;
      *dev = t.dev;
      return JV_OK;
    }
  if ((int)w.tabs.size() >= LV_CACHE) {
    size_t old = 0;
    for (size_t i = 1; i < w.tabs.size(); ++i)
      if (w.tabs[i].used < w.tabs[old].used) old = i;
    JV_HIP(hipDeviceSynchronize());      // a queued launch may still read it
    (void)hipFree(w.tabs[old].dev);
    w.tabs.erase(w.tabs.begin() + (long)old);
  }
  std::vector<double> host(2 * LV_TAB);
  level_tables(k, host.data());
  LevelTab t;
  t.fs = fs;
  t.used = w.clock;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&t.dev), host.size() * sizeof(double)));
  const hipError_t e = hipMemcpy(t.dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    return fail(JV_ERR_HIP, std::string("jv_loudness: table upload: ") + hipGetErrorString(e));
  }
  w.tabs.push_back(t);
  *dev = t.dev;
  return JV_OK;
}

}  // namespace

int trim_bounds(Context& c, const float* wav, const int* lens, int B, int n, float top_db, int F, int H, int* start, int* end,
                hipStream_t st) {
  char msg[200];
  if (!(top_db > 0.f) || !isfinite(top_db)) {
    snprintf(msg, sizeof msg, "jv_trim_bounds: top_db must be positive and finite, got %g", (double)top_db);
    return fail(JV_ERR_ARG, msg);
  }
  if (F < 1 || F > LV_MAX_FRAME || H < 1) {
    snprintf(msg, sizeof msg, "jv_trim_bounds: need 1 <= frame_length <= %d and hop_length >= 1, got %d and %d", LV_MAX_FRAME, F, H);
    return fail(JV_ERR_ARG, msg);
  }
  if (B < 0 || n < 0) return fail(JV_ERR_ARG, "jv_trim_bounds: negative size");
  if (B == 0) return JV_OK;
  if ((n > 0 && !wav) || !start || !end) return fail(JV_ERR_ARG, "jv_trim_bounds: null argument");
  const long span = (long)n + 2 * (F / 2) - F;
  const long Tmax = (n == 0 || span < 0) ? 0 : 1 + span / H;
  const long tiles = Tmax > 0 ? cdivl(Tmax, 4) : 1, per = Tmax > 0 ? cdivl(Tmax, LV_THREADS) : 1;
  if (tiles * B > LV_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_trim_bounds: too many frames for one launch");
  LevelWs& w = get(c);
  JV_TRY(scratch_reserve(w, ((size_t)3 * B + (size_t)B * Tmax) * 4));
  TrimArgs a;
  a.wav = wav; a.lens = lens; a.n = n; a.F = F; a.H = H; a.Tmax = (int)Tmax; a.tiles = (int)tiles;
  a.thr = (float)pow(10.0, -(double)top_db / 10.0);
  a.mx = static_cast<unsigned*>(w.scratch);
  a.first = reinterpret_cast<int*>(a.mx + B);
  a.last = a.first + B;
  a.ms = reinterpret_cast<float*>(a.last + B);
  a.start = start; a.end = end;
  const unsigned gb = (unsigned)cdiv(B, 64);
  hipLaunchKernelGGL(trim_init_kernel, dim3(gb), dim3(64), 0, st, a, B);
  if (Tmax > 0) {
    hipLaunchKernelGGL(trim_energy_kernel, dim3((unsigned)(tiles * B)), dim3(LV_THREADS), 0, st, a);
    hipLaunchKernelGGL(trim_mark_kernel, dim3((unsigned)(per * B)), dim3(LV_THREADS), 0, st, a, (int)per);
  }
  hipLaunchKernelGGL(trim_finish_kernel, dim3(gb), dim3(64), 0, st, a, B);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int peak(Context&, const float* wav, const int* lens, const int* start, const int* end, int B, int n, float* out, hipStream_t st) {
  if (B < 0 || n < 0) return fail(JV_ERR_ARG, "jv_peak: negative size");
  if (B == 0) return JV_OK;
  if ((n > 0 && !wav) || !out) return fail(JV_ERR_ARG, "jv_peak: null argument");
  const long tiles = n > 0 ? cdivl(n, LV_TILE) : 1;
  if (tiles * B > LV_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_peak: too many samples for one launch");
  JV_HIP(hipMemsetAsync(out, 0, (size_t)B * sizeof(float), st));
  if (n > 0)
    hipLaunchKernelGGL(peak_kernel, dim3((unsigned)(tiles * B)), dim3(LV_THREADS), 0, st, wav, lens, start, end, n, (int)tiles,
                       reinterpret_cast<unsigned*>(out));
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int loudness(Context& c, const float* wav, const int* lens, int B, int n, int fs, float* lufs, hipStream_t st) {
  if (!rate_ok(fs)) {
    char msg[128];
    snprintf(msg, sizeof msg, "jv_loudness: sample rate must lie in [8000, 192000], got %d", fs);
    return fail(JV_ERR_ARG, msg);
  }
  if (B < 0 || n < 0) return fail(JV_ERR_ARG, "jv_loudness: negative size");
  if (B == 0) return JV_OK;
  if ((n > 0 && !wav) || !lufs) return fail(JV_ERR_ARG, "jv_loudness: null argument");
  LoudArgs a;
  a.wav = wav; a.lens = lens; a.n = n; a.h = block_hop(fs); a.lufs = lufs;
  const long groups = n > 0 ? cdivl(n, LV_GSPAN) : 1;
  if (groups * B > LV_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_loudness: too many samples for one launch");
  a.groups = (int)groups;
  a.nbin = n / a.h + 1;
  a.k = kweight(fs);
  a.abs_thr = pow(10.0, (-70.0 + 0.691) / 10.0);
  LevelWs& w = get(c);
  JV_TRY(level_table(w, fs, a.k, &a.tab));
  const size_t per = (size_t)groups * LV_THREADS * 6 + (size_t)groups * 4 * 8 + (size_t)a.nbin;      // doubles per recording
  JV_TRY(scratch_reserve(w, per * B * sizeof(double)));
  a.seg = static_cast<double*>(w.scratch);
  a.sums = a.seg + (size_t)B * groups * LV_THREADS * 4;
  a.wend = a.sums + (size_t)B * groups * LV_THREADS * 2;
  a.wst = a.wend + (size_t)B * groups * 16;
  a.bins = a.wst + (size_t)B * groups * 16;
  const bool prof = prof_on();
  const double samples = (double)B * n;
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(loud_scan_kernel, dim3((unsigned)(groups * B)), dim3(LV_THREADS), 0, st, a);
  if (prof) prof_end(st, "loud_scan", 2.0 * 11 * samples, 4.0 * samples + 32.0 * samples / LV_SEG);
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(loud_carry_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
  if (prof) prof_end(st, "loud_carry", 2.0 * 16 * 8 * samples / LV_WSPAN, 64.0 * samples / LV_WSPAN);
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(loud_bins_kernel, dim3((unsigned)(groups * B)), dim3(LV_THREADS), 0, st, a);
  if (prof) prof_end(st, "loud_bins", 2.0 * 12 * samples, 4.0 * samples + 48.0 * samples / LV_SEG);
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
  if (prof) prof_end(st, "loud_gate", 2.0 * samples / LV_SEG, 16.0 * samples / LV_SEG);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int level_gain(Context&, const float* lufs, const float* pk, int B, double target, double ceiling, float* gain, hipStream_t st) {
  char msg[200];
  if (B < 0) return fail(JV_ERR_ARG, "jv_level_gain: negative size");
  if (!lufs) {
    if (!pk || !(ceiling > 0.0) || !isfinite(ceiling)) {
      snprintf(msg, sizeof msg, "jv_level_gain: without lufs (the prompt rule) peak and a positive finite ceiling are needed, got %g",
               ceiling);
      return fail(JV_ERR_ARG, msg);
    }
  } else {
    if (!isfinite(target)) {
      snprintf(msg, sizeof msg, "jv_level_gain: target_lufs must be finite, got %g", target);
      return fail(JV_ERR_ARG, msg);
    }
    if (!isfinite(ceiling) || (ceiling > 0.0 && !pk)) {
      snprintf(msg, sizeof msg, "jv_level_gain: a ceiling (%g) must be finite and needs peak", ceiling);
      return fail(JV_ERR_ARG, msg);
    }
  }
  if (B == 0) return JV_OK;
  if (!gain) return fail(JV_ERR_ARG, "jv_level_gain: null argument");
  hipLaunchKernelGGL(gain_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, lufs, pk, B, target, ceiling, gain);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int level_apply(Context&, const float* wav, const int* lens, const int* start, const int* end, const float* gain, int B, int n,
                int tail, float* out, long n_out, int* out_lens, hipStream_t st) {
  char msg[160];
  if (B < 0 || n < 0 || tail < 0 || n_out < 0) return fail(JV_ERR_ARG, "jv_level_apply: negative size");
  if (n_out < (long)n + tail) {
    snprintf(msg, sizeof msg, "jv_level_apply: n_out = %ld, but n + tail = %d + %d", n_out, n, tail);
    return fail(JV_ERR_SHAPE, msg);
  }
  if (out_lens && (long)n + tail > 0x7fffffffL) return fail(JV_ERR_SHAPE, "jv_level_apply: output lengths beyond int32 (out_lens)");
  if (B == 0) return JV_OK;
  if ((n > 0 && !wav) || (n_out > 0 && !out)) return fail(JV_ERR_ARG, "jv_level_apply: null argument");
  const long tiles = n_out > 0 ? cdivl(n_out, LV_TILE) : 1;
  if (tiles * B > LV_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_level_apply: too many output samples for one launch");
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)(tiles * B)), dim3(LV_THREADS), 0, st, wav, lens, start, end, gain, n, tail, out,
                     n_out, out_lens, (int)tiles);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

}  // namespace jv

extern "C" {

int jv_kweight_coeffs(int fs, double* out) {
  if (!jv::rate_ok(fs)) return jv::fail(JV_ERR_ARG, "jv_kweight_coeffs: sample rate must lie in [8000, 192000]");
  if (!out) return jv::fail(JV_ERR_ARG, "jv_kweight_coeffs: null argument");
  const jv::KWeight k = jv::kweight(fs);
  const double v[10] = {k.sb0, k.sb1, k.sb2, k.sa1, k.sa2, k.hb0, k.hb1, k.hb2, k.ha1, k.ha2};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
  return JV_OK;
}

int64_t jv_loudness_blocks(int64_t n, int fs) {
  if (!jv::rate_ok(fs)) return -1;
  const int64_t h = jv::block_hop(fs);
  return n < 4 * h ? 0 : (n - 4 * h) / h + 1;
}

#define JV_LEVEL_ENTER(who)                                                                                        \
  if (!ctx) return jv::fail(JV_ERR_ARG, who ": null context");                                                     \
  if (ctx->c.broken) return jv::fail(JV_ERR_STATE, who ": context unusable (jv_reserve); destroy it");             \
  JV_HIP(hipSetDevice(ctx->c.device))

int jv_trim_bounds(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, float top_db, int frame_length,
                   int hop_length, int32_t* start, int32_t* end, void* stream) {
  JV_LEVEL_ENTER("jv_trim_bounds");
  return jv::trim_bounds(ctx->c, wav, lens, B, n, top_db, frame_length, hop_length, start, end, static_cast<hipStream_t>(stream));
}

int jv_peak(jv_context* ctx, const float* wav, const int32_t* lens, const int32_t* start, const int32_t* end, int B, int n,
            float* peak, void* stream) {
  JV_LEVEL_ENTER("jv_peak");
  return jv::peak(ctx->c, wav, lens, start, end, B, n, peak, static_cast<hipStream_t>(stream));
}

int jv_loudness(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, int fs, float* lufs, void* stream) {
  JV_LEVEL_ENTER("jv_loudness");
  return jv::loudness(ctx->c, wav, lens, B, n, fs, lufs, static_cast<hipStream_t>(stream));
}

int jv_level_gain(jv_context* ctx, const float* lufs, const float* peak, int B, double target_lufs, double ceiling, float* gain,
                  void* stream) {
  JV_LEVEL_ENTER("jv_level_gain");
  return jv::level_gain(ctx->c, lufs, peak, B, target_lufs, ceiling, gain, static_cast<hipStream_t>(stream));
}

int jv_level_apply(jv_context* ctx, const float* wav, const int32_t* lens, const int32_t* start, const int32_t* end,
                   const float* gain, int B, int n, int tail, float* out, int64_t n_out, int32_t* out_lens, void* stream) {
  JV_LEVEL_ENTER("jv_level_apply");
  return jv::level_apply(ctx->c, wav, lens, start, end, gain, B, n, tail, out, (long)n_out, out_lens,
                         static_cast<hipStream_t>(stream));
}

}  // extern "C"
