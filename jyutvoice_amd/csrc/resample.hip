// Sample-rate conversion on the GPU: the two `torchaudio.transforms.Resample(orig, new)` of infer.py:368-382, i.e.
// torchaudio.functional.resample with its defaults (sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99), restated in
// include/jyutvoice_hip.h (unpinned: torchaudio is not part of this build).  With g = gcd(orig, new), o = orig / g, n = new / g:
//
//   y[i n + p] = sum_{k < K} tab[p][k] x[i o + k - width],  x = 0 outside [0, L),  K = 2 width + o
//
// a polyphase FIR: n phases of K taps, one input frame of o samples per n output samples.  About 2 K flops per output sample and no
// reuse a matrix core could take: the bound is the table and LDS reads.
//
// One launch serves a ragged batch.  A workgroup owns a run of `tile` consecutive output samples of one recording and stages the
// input span they need into LDS, SELECTING zero outside [0, len_b) -- what lies behind a length may be NaN and is never read.
// Lane l takes output j0 + l (+ 256 r): consecutive lanes are consecutive phases, so the table is kept phase-minor ([k][p]) in
// global memory and a wave's table read is one run of consecutive addresses; it is at most 4 MiB and stays in L2.
//
// LDS layout.  Tap k of frame f is span word f o + k.  Stored as it comes, a wave with n = 1 (lane l = frame l) would read a
// stride of o words, gcd(o, 32) lanes of a 32-lane group on one of the 32 banks of ds_read_b32 whatever k is (2-way for
// 48 -> 24 kHz).  The span is therefore stored de-interleaved, word i at (i mod o) S + i / o with S >= frames of the span: tap
// k = d o + c of frame f sits at c S + d + f, so at every k the lanes of a wave read f-consecutive words -- one word per frame,
// lanes of one frame the same word (a broadcast), and a 32-lane group touches at most 32 consecutive words, i.e. 32 different
// banks.  By the bank rule that is conflict-free for every (o, n, k); computed from the rule, not measured with a counter.  S is
// odd, which spreads the staging WRITES (stride S between consecutive lanes; one write per input word against K reads per
// output, so they are not what bounds the kernel).  c and d depend on k alone, so the address arithmetic is wave-uniform.
//
// Every output sample is one chain of K fmaf in ascending k, taps outside the recording included (as selected zeros): the order
// does not depend on the sample's place in the batch, the tile or the grid, nor on the tile size or the staging path, so a
// recording's samples are the same bits alone and in any batch.
#include <math.h>
#include <stdio.h>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"

namespace jv {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;               // output samples per workgroup (halved while the span does not fit)
constexpr int RS_LDS_FLOATS = 15360;        // 60 KiB of dynamic LDS at most
constexpr long RS_TABLE_CAP = 1L << 20;     // entries (n K) of a reduced pair's table
constexpr int RS_CACHE = 8;                 // tables kept per context
constexpr long RS_MAX_GROUPS = (1L << 32) / RS_THREADS - 1;      // a launch holds fewer than 2^32 threads

struct ResampleGeo { int o = 0, n = 0, width = 0, K = 0; };

struct ResampleTab {
  ResampleGeo g;
  float* dev = nullptr;     // [K][n], phase-minor
  unsigned long used = 0;   // stamp of the last call that took it (the oldest goes when the cache is full)
};

struct ResampleWs {
  std::vector<ResampleTab> tabs;
  unsigned long clock = 0;
};

void resample_ws_destroy(Context& c) {
  if (!c.rws) return;
  for (ResampleTab& t : c.rws->tabs) (void)hipFree(t.dev);
  delete c.rws;
  c.rws = nullptr;
}

namespace {

int gcd_int(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// o, n, width, K of a rate pair (both > 0); JV_ERR_ARG when the table would exceed the cap
int resample_geo(const char* who, int orig, int neu, ResampleGeo& g) {
  const int d = gcd_int(orig, neu);
  g.o = orig / d;
  g.n = neu / d;
  const double base = 0.99 * (double)(g.o < g.n ? g.o : g.n);
  const double width = ceil(6.0 * (double)g.o / base);
  const double entries = (double)g.n * (2.0 * width + (double)g.o);
  if (entries > (double)RS_TABLE_CAP) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %d -> %d Hz reduces to o = %d, n = %d, whose table of n (2 width + o) = %.0f entries exceeds the cap of %ld",
             who, orig, neu, g.o, g.n, entries, RS_TABLE_CAP);
    return fail(JV_ERR_ARG, msg);
  }
  g.width = (int)width;
  g.K = 2 * g.width + g.o;
  return JV_OK;
}

// tab[p][k] = h((k - width) / o - p / n) in fp64, rounded once; stored at tab[p * sp + k * sk]
void resample_fill(const ResampleGeo& g, float* tab, long sp, long sk) {
  const double base = 0.99 * (double)(g.o < g.n ? g.o : g.n);
  const double scale = base / (double)g.o, on = (double)g.o * (double)g.n;
  for (int p = 0; p < g.n; ++p)
    for (int k = 0; k < g.K; ++k) {
      // tau = (k - width) / o - p / n over the common denominator: the numerator is an exact integer
      const long num = (long)(k - g.width) * g.n - (long)p * g.o;
      const double u = base * ((double)num / on);
      double v = 0.0;
      if (fabs(u) <= 6.0) {
        const double w = cos(M_PI * u / 12.0);
        v = scale * (num == 0 ? 1.0 : sin(M_PI * u) / (M_PI * u)) * w * w;
      }
      tab[p * sp + k * sk] = (float)v;
    }
}

struct ResampleArgs {
  const float* wav;
  const int* lens;
  int n_in;
  float* out;
  long n_out;
  int* out_lens;
  const float* tab;   // [K][n]
  int o, n, width, K;
  int tile, tiles;    // output samples per workgroup, workgroups per recording
  int S;              // LDS row length: frames a tile's span can touch, made odd (o S floats are staged)
  int use_lds;        // 0: the span of one tile does not fit in LDS (K beyond ~15 k taps): taps are read from global memory
};

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleArgs a) {
  extern __shared__ float xs[];
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int len = a.lens ? min(max(a.lens[b], 0), a.n_in) : a.n_in;
  const long out_len = ((long)a.n * len + a.o - 1) / a.o;
  if (tile == 0 && threadIdx.x == 0 && a.out_lens) a.out_lens[b] = (int)out_len;
  const long j0 = (long)tile * a.tile;
  const long jend = min(j0 + a.tile, a.n_out);      // what this workgroup writes ...
  const long j1 = min(jend, out_len);               // ... and what of it is signal (the rest is zeros)
  const float* __restrict__ x = a.wav + (long)b * a.n_in;
  float* __restrict__ y = a.out + (long)b * a.n_out;
  const long i_lo = j0 / a.n;                       // first input frame of the tile
  const int r0 = (int)(j0 - i_lo * a.n);            // phase of the tile's first sample
  if (a.use_lds) {
    if (j1 > j0) {
      const long i_hi = (j1 - 1) / a.n;
      // (span - 1) / o = (i_hi - i_lo) + (K - 1) / o <= ceil((tile - 1) / n) + (K - 1) / o < S: what the launcher sized LDS for
      const int span = (int)(i_hi - i_lo) * a.o + a.K;
      const long s0 = i_lo * a.o - a.width;
      for (int idx = threadIdx.x; idx < span; idx += RS_THREADS) {
        const long g = s0 + idx;
        const int q = idx / a.o;
        xs[(idx - q * a.o) * a.S + q] = (g >= 0 && g < len) ? x[g] : 0.f;
      }
    }
    __syncthreads();
  }
  for (int d = threadIdx.x; j0 + d < jend; d += RS_THREADS) {
    float acc = 0.f;
    if (j0 + d < j1) {
      const int q = r0 + d, fi = q / a.n, p = q - fi * a.n;      // frame i_lo + fi, phase p
      const float* __restrict__ t = a.tab + p;
      if (a.use_lds) {
        const float* xr = xs + fi;
        int off = 0, c = 0;      // tap k = d o + c at c S + d: both follow k alone
#pragma unroll 4
        for (int k = 0; k < a.K; ++k) {
          acc = fmaf(t[k * a.n], xr[off], acc);
          off += a.S;
          if (++c == a.o) { c = 0; off -= a.o * a.S - 1; }
        }
      } else {
        const long g0 = (i_lo + fi) * a.o - a.width;
        for (int k = 0; k < a.K; ++k) {
          const long g = g0 + k;
          acc = fmaf(t[(long)k * a.n], (g >= 0 && g < len) ? x[g] : 0.f, acc);
        }
      }
    }
    y[j0 + d] = acc;
  }
}

// equal rates: out[b, :len_b] = wav[b, :len_b], zeros behind
__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(const float* __restrict__ wav, const int* __restrict__ lens,
                                                                   int n_in, float* __restrict__ out, long n_out,
                                                                   int* __restrict__ out_lens, int tiles) {
  const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
  const int len = lens ? min(max(lens[b], 0), n_in) : n_in;
  if (tile == 0 && threadIdx.x == 0 && out_lens) out_lens[b] = len;
  const long j0 = (long)tile * RS_TILE, jend = min(j0 + RS_TILE, n_out);
  for (long j = j0 + threadIdx.x; j < jend; j += RS_THREADS) out[(long)b * n_out + j] = j < len ? wav[(long)b * n_in + j] : 0.f;
}

// the cached table of (o, n), built and uploaded on a miss (the only path of jv_resample that waits for the device)
int resample_table(Context& c, const ResampleGeo& g, const float** dev) {
  if (!c.rws) c.rws = new ResampleWs();
  ResampleWs& w = *c.rws;
  ++w.clock;
  for (ResampleTab& t : w.tabs)
    if (t.g.o == g.o && t.g.n == g.n) {
      t.used = w.clock;
      *dev = t.dev;
      return JV_OK;
    }
  if ((int)w.tabs.size() >= RS_CACHE) {
    size_t old = 0;
    for (size_t i = 1; i < w.tabs.size(); ++i)
      if (w.tabs[i].used < w.tabs[old].used) old = i;
    JV_HIP(hipDeviceSynchronize());      // a queued launch may still read it
    (void)hipFree(w.tabs[old].dev);
    w.tabs.erase(w.tabs.begin() + (long)old);
  }
  const size_t count = (size_t)g.n * g.K;
  std::vector<float> host(count);
  resample_fill(g, host.data(), 1, g.n);
  ResampleTab t;
  t.g = g;
  t.used = w.clock;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&t.dev), count * sizeof(float)));
  const hipError_t e = hipMemcpy(t.dev, host.data(), count * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    return fail(JV_ERR_HIP, std::string("jv_resample: table upload: ") + hipGetErrorString(e));
  }
  w.tabs.push_back(t);
  *dev = t.dev;
  return JV_OK;
}

}  // namespace

int resample(Context& c, const float* wav, const int* lens, int B, int n_in, int orig, int neu, float* out, long n_out,
             int* out_lens, hipStream_t st) {
  if (orig <= 0 || neu <= 0) {
    char msg[128];
    snprintf(msg, sizeof msg, "jv_resample: sample rates must be positive, got %d -> %d", orig, neu);
    return fail(JV_ERR_ARG, msg);
  }
  if (B < 0 || n_in < 0 || n_out < 0) return fail(JV_ERR_ARG, "jv_resample: negative size");
  ResampleGeo g;
  if (orig != neu) JV_TRY(resample_geo("jv_resample", orig, neu, g));
  const int64_t need = jv_resample_length(n_in, orig, neu);
  if (n_out < need) {
    char msg[160];
    snprintf(msg, sizeof msg, "jv_resample: n_out = %ld, but %d samples at %d Hz are %ld at %d Hz", n_out, n_in, orig, (long)need, neu);
    return fail(JV_ERR_SHAPE, msg);
  }
  if (out_lens && need > 0x7fffffffL) return fail(JV_ERR_SHAPE, "jv_resample: output lengths beyond int32 (out_lens)");
  if (B == 0) return JV_OK;
  if ((n_in > 0 && !wav) || (n_out > 0 && !out)) return fail(JV_ERR_ARG, "jv_resample: null argument");
  if (orig == neu) {
    const long tiles = n_out > 0 ? cdivl(n_out, RS_TILE) : 1;
    if (tiles * B > RS_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_resample: too many output samples for one launch");
    hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), 0, st, wav, lens, n_in, out, n_out,
                       out_lens, (int)tiles);
    JV_HIP(hipGetLastError());
    return JV_OK;
  }
  ResampleArgs a;
  a.wav = wav; a.lens = lens; a.n_in = n_in; a.out = out; a.n_out = n_out; a.out_lens = out_lens;
  a.o = g.o; a.n = g.n; a.width = g.width; a.K = g.K;
  // the span of a tile: its samples lie in frames 0 .. ceil((tile - 1) / n), and a frame's taps reach (K - 1) / o rows further
  auto lds_rows = [&](int tile) { return (long)(((tile - 1 + g.n - 1) / g.n + (g.K - 1) / g.o + 1) | 1); };
  auto lds_floats = [&](int tile) { return lds_rows(tile) * g.o; };
  a.tile = RS_TILE;
  while (a.tile > RS_THREADS && lds_floats(a.tile) > RS_LDS_FLOATS) a.tile /= 2;
  a.use_lds = lds_floats(a.tile) <= RS_LDS_FLOATS ? 1 : 0;
  a.S = (int)lds_rows(a.tile);
  const long tiles = n_out > 0 ? cdivl(n_out, a.tile) : 1;
  if (tiles * B > RS_MAX_GROUPS) return fail(JV_ERR_SHAPE, "jv_resample: too many output samples for one launch");
  a.tiles = (int)tiles;
  JV_TRY(resample_table(c, g, &a.tab));
  const size_t lds = a.use_lds ? (size_t)lds_floats(a.tile) * sizeof(float) : 0;
  const bool prof = prof_on();
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), lds, st, a);
  if (prof) prof_end(st, "resample", 2.0 * g.K * (double)need * B, 4.0 * B * ((double)n_in + (double)n_out));
  JV_HIP(hipGetLastError());
  return JV_OK;
}

}  // namespace jv

extern "C" {

int64_t jv_resample_length(int64_t n, int orig_freq, int new_freq) {
  if (n < 0 || orig_freq <= 0 || new_freq <= 0) return -1;
  if (orig_freq == new_freq) return n;
  const int d = jv::gcd_int(orig_freq, new_freq);
  const unsigned __int128 o = (unsigned)(orig_freq / d), m = (unsigned)(new_freq / d);
  const unsigned __int128 r = (m * (unsigned __int128)(uint64_t)n + o - 1) / o;
  return r > (unsigned __int128)INT64_MAX ? -1 : (int64_t)r;
}

int jv_resample_table(int orig_freq, int new_freq, float* tab, int64_t cap, int32_t* o, int32_t* n, int32_t* width) {
  if (orig_freq <= 0 || new_freq <= 0) return jv::fail(JV_ERR_ARG, "jv_resample_table: sample rates must be positive");
  jv::ResampleGeo g;
  JV_TRY(jv::resample_geo("jv_resample_table", orig_freq, new_freq, g));
  if (o) *o = g.o;
  if (n) *n = g.n;
  if (width) *width = g.width;
  if (!tab) return JV_OK;
  if (cap < (int64_t)g.n * g.K) return jv::fail(JV_ERR_SHAPE, "jv_resample_table: cap is smaller than n (2 width + o)");
  jv::resample_fill(g, tab, g.K, 1);
  return JV_OK;
}

int jv_resample(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n_in, int orig_freq, int new_freq, float* out,
                int64_t n_out, int32_t* out_lens, void* stream) {
  if (!ctx) return jv::fail(JV_ERR_ARG, "jv_resample: null context");
  if (ctx->c.broken) return jv::fail(JV_ERR_STATE, "jv_resample: context unusable (jv_reserve); destroy it");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::resample(ctx->c, wav, lens, B, n_in, orig_freq, new_freq, out, (long)n_out, out_lens, static_cast<hipStream_t>(stream));
}

}  // extern "C"
