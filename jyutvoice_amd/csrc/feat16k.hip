// The two 16 kHz features of a reference recording (infer.py:98-163), each as ONE fused launch for a ragged batch:
//
//   fbank        kaldi.fbank(speech, num_mel_bins=80, dither=0, sample_frequency=16000) [- its mean over frames]   -> [B, Tmax, 80]
//   whisper      whisper.log_mel_spectrogram(audio, n_mels=128)                                                     -> [B, 128, Tmax]
//
// Both are restated in include/jyutvoice_hip.h (unpinned: torchaudio and whisper are not part of this build).  Both are
// frames of 400 samples every 160, conditioned in fp32, a DFT as a product against a cos | -sin basis, |.|^2, a mel
// projection and a log; then one reduction over the recording's own frames (fbank: the mean per bin; Whisper: the maximum).
//
// Ownership.  A workgroup (4 waves) owns FK_TILE = 32 consecutive frames of one recording; tiles are enumerated over
// B x ceil(Tmax / 32) and lengths are read on the device, so the call enqueues two launches and never synchronises.  A tile
// behind its recording's frame count writes zeros and leaves.
//
// LDS (dynamic, 73 152 B: two workgroups per CU).
//   span  [5360]       the tile's samples, staged once, SELECTING zero outside [0, len_b); Whisper's reflect index is taken at the
//                      recording's own ends before the select.  Nothing behind len_b is read, so it may be NaN.
//   A     [32][404]    the conditioned frames (fbank: minus the frame mean, pre-emphasis, Povey window; Whisper: Hann window).
//   P     [32][260]    the power spectrum, laid over A once every wave has finished its DFT columns.
//   L     [32][129]    the log-mel values, laid over the span, from which the tile's rows and its partial are written.
// Bank rule.  A and P are read as the A operand of the f32 MFMA with ds_read_b128: lane (r = l & 31, h = l >> 5) reads the four
// words [r][8 q + 4 h ..].  ds_read_b128 is served in four groups of 16 lanes over 64 banks; each group holds 16 rows whose
// r mod 16 are all different, one h.  With a row stride S, S / 4 odd (404 / 4 = 101, 260 / 4 = 65), r S / 4 mod 16 is a permutation
// of those 16 rows onto the 16 four-bank slots: conflict-free.  Conditioning writes A and reads the span with consecutive
// lanes on consecutive words (ds_*_b32, 32 banks: conflict-free); the power writes put the 32 lanes of a half on 32 consecutive
// words of one row.  L has stride 129: the Whisper read-out walks frames along lanes (bank (fr + m) mod 32), the fbank one
// walks bins.  Computed from the rule, not measured with a counter.
//
// The two products run on v_mfma_f32_32x32x2_f32, which rounds as an fmaf chain.  The operands are stored k-minor in groups of
// four (basis [100][bins][cos 4 | -sin 4], mel weights [bins / 4][mels][4]) so that a lane's four k come as one 16-byte load
// beside the 16-byte A read: MFMA i of block q sums k = 8 q + i (lanes 0-31) and k = 8 q + 4 + i (lanes 32-63).  That order is a
// property of the kernel alone -- not of the tile, the batch position or the grid -- so a frame gives the same bits wherever it
// lies.  K and N are padded with zero WEIGHTS (bins up to a multiple of 32, mels up to 96), never by reading past a row.
// fbank's Nyquist bin has weight 0 in every bank (include/jyutvoice_hip.h), so its 256 columns are bins 0 .. 255.
//
// Per-recording reductions.  The kernel writes the log values and one partial per tile (fbank: 80 column sums over the tile's
// frames, ascending; Whisper: the tile's maximum).  feat16k_finish reduces a recording's partials in ascending tile order and
// applies the mean subtraction, or max(L, max - 8) and (L + 4) / 4, in place.  No atomics: tiles start at the recording's frame
// 0, so the mean has the same bits alone and in a batch.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"

namespace jv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FK_THREADS = 256;
constexpr int FK_TILE = 32;                                   // frames per workgroup
constexpr int FK_WIN = 400, FK_HOP = 160;
constexpr int FK_SPAN = (FK_TILE - 1) * FK_HOP + FK_WIN;      // 5360 samples
constexpr int FK_AS = 404, FK_PS = 260, FK_LS = 129;          // row strides of the A, power and log images
constexpr int FK_LDS_FLOATS = FK_SPAN + FK_TILE * FK_AS;
constexpr int FK_KQ = FK_WIN / 4;                             // k groups of the DFT
constexpr int FK_FBANK = 0, FK_WHISPER = 1;
constexpr long FK_MAX_GROUPS = (1L << 24) - 1;

static_assert(FK_TILE * FK_PS <= FK_TILE * FK_AS, "the power image lies over the A image");
static_assert(FK_TILE * FK_LS + 4 <= FK_SPAN, "the log image and the maximum's scratch lie over the span");
static_assert((FK_SPAN * 4) % 16 == 0 && (FK_AS / 4) % 2 == 1 && (FK_PS / 4) % 2 == 1, "ds_read_b128: alignment and the bank rule");

template <int FEAT> struct FeatGeo;
template <> struct FeatGeo<FK_FBANK> {
  static constexpr int NFFT = 512, BINS = 256, NB = 256, NMEL = 80, MELP = 96, PW = 80, PAD = 0;
};
template <> struct FeatGeo<FK_WHISPER> {
  static constexpr int NFFT = 400, BINS = 201, NB = 224, NMEL = 128, MELP = 128, PW = 1, PAD = 200;
};

struct FeatWs {
  float* basis[2] = {nullptr, nullptr};     // [100][NB][8]
  float* win[2] = {nullptr, nullptr};       // [400]
  float* melw[2] = {nullptr, nullptr};      // [NB / 4][MELP][4]
  bool mel_ready[2] = {false, false};
  bool lds_set[2] = {false, false};
  float* part = nullptr;                    // per-tile partials of the call in flight
  size_t part_cap = 0;
};

void feat16k_ws_destroy(Context& c) {
  if (!c.fws) return;
  for (int f = 0; f < 2; ++f) {
    (void)hipFree(c.fws->basis[f]);
    (void)hipFree(c.fws->win[f]);
    (void)hipFree(c.fws->melw[f]);
  }
  (void)hipFree(c.fws->part);
  delete c.fws;
  c.fws = nullptr;
}

namespace {

__host__ __device__ inline int fbank_frames(int len) { return len < FK_WIN ? 0 : 1 + (len - FK_WIN) / FK_HOP; }
__host__ __device__ inline int whisper_frames(int len) { return len <= 200 ? 0 : len / FK_HOP; }

double kaldi_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

// bank b, bin k of the 512-point spectrum (k <= 256), in fp64
double kaldi_bank(int b, int k) {
  if (k >= 256) return 0.0;
  const double lo = kaldi_mel(20.0), hi = kaldi_mel(8000.0), d = (hi - lo) / 81.0;
  const double left = lo + b * d, centre = lo + (b + 1) * d, right = lo + (b + 2) * d;
  const double m = kaldi_mel(31.25 * k);
  const double up = (m - left) / (centre - left), down = (right - m) / (right - centre);
  const double w = up < down ? up : down;
  return w > 0.0 ? w : 0.0;
}

// window and DFT basis of one feature, in fp64 with an exact integer angle modulus, rounded once
template <int FEAT>
__global__ __launch_bounds__(256) void feat16k_basis_kernel(float* __restrict__ basis, float* __restrict__ win) {
  using G = FeatGeo<FEAT>;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < FK_WIN) {
    const double den = FEAT == FK_FBANK ? 399.0 : 400.0;
    const double hann = 0.5 - 0.5 * cos(2.0 * M_PI * (double)idx / den);
    win[idx] = (float)(FEAT == FK_FBANK ? pow(hann, 0.85) : hann);
  }
  if (idx >= FK_KQ * G::NB * 8) return;
  const int kq = idx / (G::NB * 8), rem = idx - kq * (G::NB * 8), bin = rem >> 3, j = rem & 7;
  const int k = 4 * kq + (j & 3);
  float v = 0.f;
  if (bin < G::BINS) {
    const double ang = 2.0 * M_PI * (double)((bin * k) % G::NFFT) / (double)G::NFFT;
    v = (float)(j < 4 ? cos(ang) : -sin(ang));
  }
  basis[idx] = v;
}

// [128][201] filterbank -> [56][128][4], bins 201 .. 223 zero
__global__ __launch_bounds__(256) void feat16k_pack_filters_kernel(const float* __restrict__ src, float* __restrict__ dst) {
  using G = FeatGeo<FK_WHISPER>;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= G::NB * G::MELP) return;
  const int kq = idx / (G::MELP * 4), rem = idx - kq * (G::MELP * 4), m = rem >> 2, bin = 4 * kq + (rem & 3);
  dst[idx] = bin < 201 ? src[m * 201 + bin] : 0.f;
}

struct FeatArgs {
  const float* wav;
  const int* lens;
  int n;
  float* out;
  int* out_lens;
  int Tmax, tiles;
  const float *basis, *win, *melw;
  float* part;
};

template <int FEAT>
__global__ __launch_bounds__(FK_THREADS) void feat16k_kernel(FeatArgs a) {
  using G = FeatGeo<FEAT>;
  extern __shared__ __attribute__((aligned(16))) float fk_lds[];
  float* span = fk_lds;
  float* A = fk_lds + FK_SPAN;
  float* P = A;
  float* L = span;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const int T = FEAT == FK_FBANK ? fbank_frames(len) : whisper_frames(len);
  if (tile == 0 && tid == 0 && a.out_lens) a.out_lens[b] = T;
  const int f0 = tile * FK_TILE;
  const int nrows = min(FK_TILE, a.Tmax - f0);            // rows of the output this tile owns
  const int nvalid = min(max(T - f0, 0), nrows);          // ... and how many of them are frames of the recording
  if (nvalid == 0) {
    if (FEAT == FK_FBANK) {
      for (int idx = tid; idx < nrows * G::NMEL; idx += FK_THREADS) a.out[((long)b * a.Tmax + f0) * G::NMEL + idx] = 0.f;
    } else {
      for (int idx = tid; idx < G::NMEL * FK_TILE; idx += FK_THREADS) {
        const int m = idx >> 5, fr = idx & 31;
        if (fr < nrows) a.out[((long)b * G::NMEL + m) * a.Tmax + f0 + fr] = 0.f;
      }
    }
    return;
  }

  // ---- the tile's samples, once; rows behind the recording's frames see selected zeros too ----
  const float* __restrict__ x = a.wav + (long)b * a.n;
  const long s0 = (long)f0 * FK_HOP - G::PAD;
  for (int idx = tid; idx < FK_SPAN; idx += FK_THREADS) {
    long j = s0 + idx;
    if (FEAT == FK_WHISPER) {
      if (j < 0) j = -j;
      if (j >= len) j = 2L * (len - 1) - j;
    }
    span[idx] = (j >= 0 && j < len) ? x[j] : 0.f;
  }
  __syncthreads();

  // ---- conditioning: a wave takes 8 frames, one after the other; lane l holds samples l, l + 64, ... ----
  {
    float w[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) w[j] = lane + 64 * j < FK_WIN ? a.win[lane + 64 * j] : 0.f;
    for (int fr = 0; fr < 8; ++fr) {
      const int r = 8 * wave + fr;
      const float* xr = span + FK_HOP * r;
      float* ar = A + FK_AS * r;
      if (FEAT == FK_FBANK) {
        float s = 0.f;      // the frame's mean: 7 ascending terms per lane, then a butterfly (the same order for every frame)
#pragma unroll
        for (int j = 0; j < 7; ++j) s += lane + 64 * j < FK_WIN ? xr[lane + 64 * j] : 0.f;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)FK_WIN;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          if (i < FK_WIN) {
            const float d = xr[i] - mean, dp = xr[i > 0 ? i - 1 : 0] - mean;      // a[-1] := a[0]
            ar[i] = (d - 0.97f * dp) * w[j];
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          if (i < FK_WIN) ar[i] = xr[i] * w[j];
        }
      }
    }
  }
  __syncthreads();

  // ---- DFT: a wave takes bin tiles wave, wave + 4; re and im of a bin in one lane, the power formed in registers ----
  constexpr int NT = G::NB / 32;
  f32x16 pw[2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int t = wave + 4 * ti;
    if (t < NT) {
      f32x16 re, im;
#pragma unroll
      for (int e = 0; e < 16; ++e) re[e] = im[e] = 0.f;
      const float* ap = A + FK_AS * c + 4 * h;
      const f32x4* bp = reinterpret_cast<const f32x4*>(a.basis) + ((long)h * G::NB + t * 32 + c) * 2;
#pragma unroll 5
      for (int q = 0; q < FK_KQ / 2; ++q) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * q);
        const f32x4 cv = bp[(long)q * (4 * G::NB)], sv = bp[(long)q * (4 * G::NB) + 1];
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, cv.x, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, sv.x, im, 0, 0, 0);
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, cv.y, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, sv.y, im, 0, 0, 0);
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, cv.z, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, sv.z, im, 0, 0, 0);
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, cv.w, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, sv.w, im, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) pw[ti][e] = re[e] * re[e] + im[e] * im[e];
    }
  }
  __syncthreads();      // A is dead: the power image goes over it
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int t = wave + 4 * ti;
    if (t < NT) {
#pragma unroll
      for (int e = 0; e < 16; ++e) P[((e & 3) + 8 * (e >> 2) + 4 * h) * FK_PS + t * 32 + c] = pw[ti][e];
    }
  }
  __syncthreads();

  // ---- mel projection and the log; the span is dead: the log image goes over it ----
  for (int mt = wave; mt < G::MELP / 32; mt += 4) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const float* pp = P + FK_PS * c + 4 * h;
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.melw) + ((long)h * G::MELP + mt * 32 + c);
#pragma unroll 4
    for (int q = 0; q < G::NB / 8; ++q) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pp + 8 * q);
      const f32x4 wv = wp[(long)q * (2 * G::MELP)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.x, wv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.y, wv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.z, wv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.w, wv.w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      // on the floor the log is the correctly rounded constant (log(2^-23), log10(1e-10) = -10), not the device logf's value of it
      const float v = FEAT == FK_FBANK ? (acc[e] > 1.1920929e-07f ? logf(acc[e]) : -15.942385152878742f)
                                       : (acc[e] > 1e-10f ? log10f(acc[e]) : -10.0f);
      L[((e & 3) + 8 * (e >> 2) + 4 * h) * FK_LS + mt * 32 + c] = v;
    }
  }
  __syncthreads();

  // ---- the tile's rows (zeros behind the recording's frames) and its partial ----
  if (FEAT == FK_FBANK) {
    float* __restrict__ o = a.out + ((long)b * a.Tmax + f0) * G::NMEL;
    for (int idx = tid; idx < nrows * G::NMEL; idx += FK_THREADS) {
      const int fr = idx / G::NMEL, m = idx - fr * G::NMEL;
      o[idx] = fr < nvalid ? L[fr * FK_LS + m] : 0.f;
    }
    if (tid < G::NMEL) {
      float s = 0.f;
      for (int fr = 0; fr < nvalid; ++fr) s += L[fr * FK_LS + tid];
      a.part[((long)b * a.tiles + tile) * G::PW + tid] = s;
    }
  } else {
    float mx = -INFINITY;
    for (int idx = tid; idx < G::NMEL * FK_TILE; idx += FK_THREADS) {
      const int m = idx >> 5, fr = idx & 31;
      if (fr < nrows) {
        const float v = fr < nvalid ? L[fr * FK_LS + m] : 0.f;
        a.out[((long)b * G::NMEL + m) * a.Tmax + f0 + fr] = v;
        if (fr < nvalid) mx = fmaxf(mx, v);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float* red = span + FK_TILE * FK_LS;
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) a.part[(long)b * a.tiles + tile] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
}

// a recording's partials in ascending tile order, then in place: fbank minus the mean over its T_b frames; Whisper
// max(L, max - 8), (L + 4) / 4.  One workgroup per tile; rows behind T_b are zeros already.
template <int FEAT>
__global__ __launch_bounds__(FK_THREADS) void feat16k_finish(FeatArgs a) {
  using G = FeatGeo<FEAT>;
  __shared__ float mean[G::NMEL];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n) : a.n;
  const int T = FEAT == FK_FBANK ? fbank_frames(len) : whisper_frames(len);
  const int f0 = tile * FK_TILE;
  const int nvalid = min(max(T - f0, 0), FK_TILE);
  if (nvalid == 0) return;
  const int nt = (T + FK_TILE - 1) / FK_TILE;
  const float* __restrict__ part = a.part + (long)b * a.tiles * G::PW;
  if (FEAT == FK_FBANK) {
    if (tid < G::NMEL) {
      float s = 0.f;
      for (int t = 0; t < nt; ++t) s += part[t * G::PW + tid];
      mean[tid] = s / (float)T;
    }
    __syncthreads();
    float* __restrict__ o = a.out + ((long)b * a.Tmax + f0) * G::NMEL;
    for (int idx = tid; idx < nvalid * G::NMEL; idx += FK_THREADS) o[idx] -= mean[idx % G::NMEL];
  } else {
    float mx = -INFINITY;
    for (int t = 0; t < nt; ++t) mx = fmaxf(mx, part[t]);
    const float floor_ = mx - 8.0f;
    for (int idx = tid; idx < G::NMEL * FK_TILE; idx += FK_THREADS) {
      const int m = idx >> 5, fr = idx & 31;
      if (fr < nvalid) {
        float* p = a.out + ((long)b * G::NMEL + m) * a.Tmax + f0 + fr;
        *p = (fmaxf(*p, floor_) + 4.0f) / 4.0f;
      }
    }
  }
}

FeatWs& get(Context& c) {
  if (!c.fws) c.fws = new FeatWs();
  return *c.fws;
}

// first call of a feature in a context: window and basis (built on the device), the launch's LDS size
template <int FEAT>
int feat_prepare(FeatWs& w, hipStream_t st) {
  using G = FeatGeo<FEAT>;
  if (!w.lds_set[FEAT]) {
    JV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&feat16k_kernel<FEAT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               FK_LDS_FLOATS * (int)sizeof(float)));
    w.lds_set[FEAT] = true;
  }
  if (!w.basis[FEAT]) {
    float *basis = nullptr, *win = nullptr;
    const int count = FK_KQ * G::NB * 8;
    JV_HIP(hipMalloc(reinterpret_cast<void**>(&basis), (size_t)count * sizeof(float)));
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&win), FK_WIN * sizeof(float));
    if (e != hipSuccess) {
      (void)hipFree(basis);
      return fail(JV_ERR_HIP, std::string("feat16k: window: ") + hipGetErrorString(e));
    }
    hipLaunchKernelGGL(feat16k_basis_kernel<FEAT>, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, st, basis, win);
    w.basis[FEAT] = basis;
    w.win[FEAT] = win;
    JV_HIP(hipGetLastError());
  }
  return JV_OK;
}

// the Kaldi banks, built on the host in fp64 and uploaded once: [64][96][4], mels 80 .. 95 zero
int fbank_banks(FeatWs& w) {
  using G = FeatGeo<FK_FBANK>;
  if (w.mel_ready[FK_FBANK]) return JV_OK;
  std::vector<float> host((size_t)G::NB * G::MELP, 0.f);
  for (int k = 0; k < G::NB; ++k)
    for (int m = 0; m < G::NMEL; ++m) host[((size_t)(k >> 2) * G::MELP + m) * 4 + (k & 3)] = (float)kaldi_bank(m, k);
  if (!w.melw[FK_FBANK]) JV_HIP(hipMalloc(reinterpret_cast<void**>(&w.melw[FK_FBANK]), host.size() * sizeof(float)));
  JV_HIP(hipMemcpy(w.melw[FK_FBANK], host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  w.mel_ready[FK_FBANK] = true;
  return JV_OK;
}

int part_reserve(FeatWs& w, size_t count) {
  if (count <= w.part_cap) return JV_OK;
  JV_HIP(hipDeviceSynchronize());      // a queued launch may still use the old one
  (void)hipFree(w.part);
  w.part = nullptr;
  w.part_cap = 0;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&w.part), count * sizeof(float)));
  w.part_cap = count;
  return JV_OK;
}

template <int FEAT>
int feat_run(Context& c, const char* who, const float* wav, const int* lens, int B, int n, bool finish, float* out, int* out_lens,
             hipStream_t st) {
  using G = FeatGeo<FEAT>;
  FeatWs& w = get(c);
  if (B < 0 || n < 0) return fail(JV_ERR_ARG, std::string(who) + ": negative size");
  if (FEAT == FK_WHISPER && !w.mel_ready[FK_WHISPER])
    return fail(JV_ERR_STATE, std::string(who) + ": filterbank not loaded (jv_load_whisper_filters)");
  const int Tmax = FEAT == FK_FBANK ? fbank_frames(n) : whisper_frames(n);
  if (!lens && Tmax == 0) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %d samples give no frame (need %s)", who, n, FEAT == FK_FBANK ? "at least 400" : "more than 200");
    return fail(JV_ERR_ARG, msg);
  }
  if (B == 0) return JV_OK;
  if ((n > 0 && !wav) || (Tmax > 0 && !out)) return fail(JV_ERR_ARG, std::string(who) + ": null argument");
  const long tiles = Tmax > 0 ? cdivl(Tmax, FK_TILE) : 1;
  if (tiles * B > FK_MAX_GROUPS) return fail(JV_ERR_SHAPE, std::string(who) + ": too many frames for one launch");
  JV_TRY(feat_prepare<FEAT>(w, st));
  if (FEAT == FK_FBANK) JV_TRY(fbank_banks(w));
  JV_TRY(part_reserve(w, (size_t)tiles * B * G::PW));
  FeatArgs a;
  a.wav = wav; a.lens = lens; a.n = n; a.out = out; a.out_lens = out_lens; a.Tmax = Tmax; a.tiles = (int)tiles;
  a.basis = w.basis[FEAT]; a.win = w.win[FEAT]; a.melw = w.melw[FEAT]; a.part = w.part;
  const bool prof = prof_on();
  const double frames = (double)B * Tmax;
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(feat16k_kernel<FEAT>, dim3((unsigned)(tiles * B)), dim3(FK_THREADS), FK_LDS_FLOATS * sizeof(float), st, a);
  if (prof)
    prof_end(st, FEAT == FK_FBANK ? "feat16k_fbank" : "feat16k_whisper", 2.0 * frames * (2.0 * FK_WIN * G::NB + (double)G::NB * G::MELP),
             4.0 * (B * (double)n + frames * G::NMEL));
  if (finish) {
    if (prof) prof_begin(st);
    hipLaunchKernelGGL(feat16k_finish<FEAT>, dim3((unsigned)(tiles * B)), dim3(FK_THREADS), 0, st, a);
    if (prof) prof_end(st, FEAT == FK_FBANK ? "feat16k_finish_fbank" : "feat16k_finish_whisper", frames * G::NMEL, 8.0 * frames * G::NMEL);
  }
  JV_HIP(hipGetLastError());
  return JV_OK;
}

int load_whisper_filters(Context& c, const float* data, bool on_device, hipStream_t st) {
  using G = FeatGeo<FK_WHISPER>;
  FeatWs& w = get(c);
  float* tmp = nullptr;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(float) * 128 * 201));
  hipError_t e = hipSuccess;
  if (!w.melw[FK_WHISPER]) {
    JV_HIP(hipDeviceSynchronize());
    e = hipMalloc(reinterpret_cast<void**>(&w.melw[FK_WHISPER]), sizeof(float) * G::NB * G::MELP);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(tmp, data, sizeof(float) * 128 * 201, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(feat16k_pack_filters_kernel, dim3((unsigned)cdiv(G::NB * G::MELP, 256)), dim3(256), 0, st, tmp, w.melw[FK_WHISPER]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(JV_ERR_HIP, std::string("jv_load_whisper_filters: ") + hipGetErrorString(e));
  w.mel_ready[FK_WHISPER] = true;
  return JV_OK;
}

}  // namespace

}  // namespace jv

extern "C" {

int64_t jv_fbank_frames(int64_t n) { return n < jv::FK_WIN ? 0 : 1 + (n - jv::FK_WIN) / jv::FK_HOP; }

int64_t jv_whisper_frames(int64_t n) { return n <= 200 ? 0 : n / jv::FK_HOP; }

int jv_kaldi_mel_banks(float* out) {
  if (!out) return jv::fail(JV_ERR_ARG, "jv_kaldi_mel_banks: null argument");
  for (int m = 0; m < 80; ++m)
    for (int k = 0; k < 257; ++k) out[m * 257 + k] = (float)jv::kaldi_bank(m, k);
  return JV_OK;
}

int jv_load_whisper_filters(jv_context* ctx, const float* data, int64_t numel, int on_device, void* stream) {
  if (!ctx || !data) return jv::fail(JV_ERR_ARG, "jv_load_whisper_filters: null argument");
  if (numel != 128 * 201) return jv::fail(JV_ERR_SHAPE, "jv_load_whisper_filters: expected 128*201 floats");
  if (ctx->c.broken) return jv::fail(JV_ERR_STATE, "jv_load_whisper_filters: context unusable (jv_reserve); destroy it");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::load_whisper_filters(ctx->c, data, on_device != 0, static_cast<hipStream_t>(stream));
}

int jv_fbank(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, int subtract_mean, float* out, int32_t* out_lens,
             void* stream) {
  if (!ctx) return jv::fail(JV_ERR_ARG, "jv_fbank: null context");
  if (ctx->c.broken) return jv::fail(JV_ERR_STATE, "jv_fbank: context unusable (jv_reserve); destroy it");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::feat_run<jv::FK_FBANK>(ctx->c, "jv_fbank", wav, lens, B, n, subtract_mean != 0, out, out_lens,
                                    static_cast<hipStream_t>(stream));
}

int jv_whisper_log_mel(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, float* out, int32_t* out_lens,
                       void* stream) {
  if (!ctx) return jv::fail(JV_ERR_ARG, "jv_whisper_log_mel: null context");
  if (ctx->c.broken) return jv::fail(JV_ERR_STATE, "jv_whisper_log_mel: context unusable (jv_reserve); destroy it");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::feat_run<jv::FK_WHISPER>(ctx->c, "jv_whisper_log_mel", wav, lens, B, n, true, out, out_lens,
                                      static_cast<hipStream_t>(stream));
}

}  // extern "C"
