// extern "C" surface of libjyutvoice_hip.so (include/jyutvoice_hip.h).  Nothing throws across it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"
#include "jv_ops.h"
#include "hiftpair_kernel.h"
#include "rowres_kernel.h"

namespace jv {

int hiftconv(const HiftConvArgs& a, int C, hipStream_t st);   // hiftconv.hip
int rowgemm(const RowGemmArgs& a, int epi, hipStream_t st);   // rowgemm.hip
int rowconv(const RowConvArgs& a, hipStream_t st);
int hiftpair(const HiftPairArgs& a, int C, hipStream_t st);   // hiftconv.hip
int hift_lds_bytes(int pair, int C, int NG, int ntaps, int dil);
int rowres(const RowResArgs& a, hipStream_t st);              // rowgemm.hip
int rowffn(const RowFfnArgs& a, hipStream_t st);
int rowblock(const RowBlockArgs& a, bool qkv, hipStream_t st);   // rowblock.hip
int rowgemm_tile(int M);

int split3_planes(const float* src, unsigned short* dst, long n, hipStream_t st);   // registry.hip
int split2h_planes(const float* src, int rows, int ld, float* stats, unsigned short* dst, float* colscale, hipStream_t st);
float h3_scale_for_bound(float bound);
int split2h_rows(const float* x, long ld, unsigned short* dst, long plane, long rows, int C, float scale, hipStream_t st,
                 long ldd = 0);   // rowops.hip

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int ws_alloc(Context& c, size_t bytes, void** out) {
  void* p = nullptr;
  bytes = (bytes + 255) & ~(size_t)255;
  JV_HIP(hipMalloc(&p, bytes));
  JV_HIP(hipMemset(p, 0, bytes));
  c.ws_allocs.push_back(p);
  *out = p;
  return JV_OK;
}

int hift_ws_create(Context& c);   // hift.hip
int enc_ws_create(Context& c);    // encoder.hip
void flow_ws_destroy(Context& c);
void hift_ws_destroy(Context& c);
void enc_ws_destroy(Context& c);

}  // namespace jv

using jv::Context;


#define CTX_GUARD(ctx)                                                       \
  if (!(ctx)) return jv::fail(JV_ERR_ARG, "null context");                   \
  if ((ctx)->c.broken) return jv::fail(JV_ERR_STATE, "context unusable: a workspace allocation failed and the previous capacities could not be restored (jv_reserve); destroy it"); \
  {                                                                          \
    hipError_t _e = hipSetDevice((ctx)->c.device);                           \
    if (_e != hipSuccess) return jv::fail(JV_ERR_HIP, hipGetErrorString(_e)); \
  }

// Everything whose size follows the capacities (max_batch, max_frames, max_tokens).  Weights (raw + packed arenas), the
// noise tensor and the mel filterbank do not: jv_reserve re-creates only this, never re-uploads or re-packs a weight.
static int workspaces_create(Context& c) {
  int rc = jv::flow_ws_create(c);
  if (rc == JV_OK) rc = jv::hift_ws_create(c);
  if (rc == JV_OK) rc = jv::enc_ws_create(c);
  return rc;
}
static void workspaces_destroy(Context& c) {
  for (void* p : c.ws_allocs) (void)hipFree(p);
  c.ws_allocs.clear();
  jv::flow_ws_destroy(c);      // also drops captured Euler-step graphs: they point into the old buffers
  jv::hift_ws_destroy(c);
  jv::enc_ws_destroy(c);
  jv::prompt_ws_destroy(c);    // sized on demand by its own calls (prompt.hip); capped by max_frames
}

// Scratch of the operator hooks (jv_op_*: test and tuning aids, but exported): one growing buffer per (device, hook slot),
// looked up under a lock, so a buffer allocated on device A is never handed out after hipSetDevice(B) and two threads cannot
// race the grow.  Calls of ONE hook on ONE device still share the buffer: the caller serialises those (stream order does).
namespace {
enum OpSlot { OPS_X6 = 0, OPS_H3, OPS_H3_A, OPS_CONV, OPS_RG, OPS_RG_A, OPS_RC, OPS_HIFT, OPS_ATTN, OPS_QKV, OPS_QKV_A, OPS_RR, OPS_HP, OPS_RB, OPS_SK, OPS_COUNT };
int op_scratch(int slot, size_t need, void** out) {
  struct Buf { void* p = nullptr; size_t cap = 0; };
  static std::mutex mu;
  static Buf bufs[64][OPS_COUNT];
  int dev = 0;
  JV_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  Buf& b = bufs[dev & 63][slot];
  if (need > b.cap) {
    if (b.p) (void)hipFree(b.p);      // (synchronises the device: nothing still reads the old buffer)
    b.p = nullptr; b.cap = 0;
    JV_HIP(hipMalloc(&b.p, need));
    b.cap = need;
  }
  *out = b.p;
  return JV_OK;
}

// layout of one hook's scratch: the same function runs once without a base (sizes only) and once over the buffer
struct Bump {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};
// a weight matrix [N][K] as the registry keeps it: fp16x3 planes + column scales (+ row statistics: max |w|, L1 norm) (+ fragment order)
struct OpW {
  int N = 0, K = 0;
  unsigned short* planes = nullptr;
  float *cs = nullptr, *stats = nullptr;
  unsigned short* wf = nullptr;
  long n() const { return (long)N * K; }
  void take(Bump& b, int N_, int K_, bool frag) {
    N = N_; K = K_;
    planes = b.take<unsigned short>(2 * (size_t)n());
    cs = b.take<float>((size_t)N);
    stats = b.take<float>(2 * (size_t)N);
    wf = frag ? b.take<unsigned short>(2 * (size_t)n()) : nullptr;
  }
  int pack(const float* W, hipStream_t st, bool frag) const {
    JV_TRY(jv::split2h_planes(W, N, K, stats, planes, cs, st));
    if (frag) JV_TRY(jv::pack_wfrag(planes, n(), K, N, K, wf, n(), st));
    return JV_OK;
  }
};
}  // namespace

namespace jv {
int zero_rows_behind(float* att, const long* len, int len_mul, int B, int T, int G, int S, hipStream_t st);   // promptops.hip
}

extern "C" {

const char* jv_last_error(void) { return jv::g_last_error.c_str(); }

int jv_create(jv_context** out, int device, int max_batch, int max_frames, int max_tokens) {
  if (!out) return jv::fail(JV_ERR_ARG, "jv_create: null out pointer");
  *out = nullptr;
  if (max_batch < 1 || max_frames < 1 || max_tokens < 1) return jv::fail(JV_ERR_ARG, "jv_create: capacities must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return jv::fail(JV_ERR_HIP, "jv_create: no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return jv::fail(JV_ERR_ARG, "jv_create: bad device index");
  JV_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  JV_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return jv::fail(JV_ERR_HIP, std::string("jv_create: built for gfx950 only, found ") + prop.gcnArchName);
  jv_context* ctx = new (std::nothrow) jv_context();
  if (!ctx) return jv::fail(JV_ERR_HIP, "jv_create: out of host memory");
  Context& c = ctx->c;
  c.device = device;
  c.max_batch = max_batch;
  c.step_graphs = getenv("JV_STEP_GRAPH") != nullptr;
  c.exact_range = getenv("JV_EXACT_RANGE") != nullptr;
  c.est_fp16 = getenv("JV_EST_FP16") != nullptr;
  if (c.est_fp16 && c.exact_range) {
    delete ctx;
    return jv::fail(JV_ERR_STATE, "jv_create: JV_EST_FP16 (one fp16 product) and JV_EXACT_RANGE (bf16x6 everywhere) contradict each other");
  }
  c.dma_a = getenv("JV_DMA_A") != nullptr;
  c.no_rowgemm = getenv("JV_NO_ROWGEMM") != nullptr;
  c.no_ffn_fuse = getenv("JV_NO_FFN_FUSE") != nullptr;
  c.no_block_fuse = getenv("JV_NO_BLOCK_FUSE") != nullptr;
  c.no_qkv_split = getenv("JV_NO_QKV_SPLIT") != nullptr;
  c.no_compact = getenv("JV_NO_COMPACT") != nullptr;
  c.no_res_fold = getenv("JV_NO_RES_FOLD") != nullptr;
  c.no_res_pair = getenv("JV_NO_RES_PAIR") != nullptr;
  c.no_res_qkv = getenv("JV_NO_RES_QKV") != nullptr;
  c.no_ln_fold = getenv("JV_NO_LN_FOLD") != nullptr;
  c.no_temb_pre = getenv("JV_NO_TEMB_PRE") != nullptr;
  c.no_cfg_share = getenv("JV_NO_CFG_SHARE") != nullptr;
  c.no_twin_drop = getenv("JV_NO_TWIN_DROP") != nullptr;
  c.no_hiftconv = getenv("JV_NO_HIFTCONV") != nullptr;
  c.no_hift_pair = getenv("JV_NO_HIFT_PAIR") != nullptr;
  c.max_frames = max_frames;
  c.max_tokens = max_tokens;
  jv::build_registry(c);
  int rc = jv::conv_gemm_init();
  if (rc == JV_OK) rc = workspaces_create(c);
  // the noise tensor is a weight-like constant: it lives outside the workspace and survives jv_reserve
  if (rc == JV_OK && hipMalloc(reinterpret_cast<void**>(&c.noise), sizeof(float) * jv::N_FEATS * jv::NOISE_FRAMES) != hipSuccess)
    rc = jv::fail(JV_ERR_HIP, "jv_create: out of device memory (noise tensor)");
  if (rc != JV_OK) {
    jv_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return JV_OK;
}

int jv_reserve(jv_context* ctx, int max_batch, int max_frames, int max_tokens) {
  CTX_GUARD(ctx);
  Context& c = ctx->c;
  if (max_batch < 1 || max_frames < 1 || max_tokens < 1) return jv::fail(JV_ERR_ARG, "jv_reserve: capacities must be >= 1");
  if (max_batch == c.max_batch && max_frames == c.max_frames && max_tokens == c.max_tokens) return JV_OK;
  JV_HIP(hipDeviceSynchronize());      // nothing queued may still use the old workspace (or replay a graph that points into it)
  const int old_b = c.max_batch, old_f = c.max_frames, old_t = c.max_tokens;
  workspaces_destroy(c);
  c.max_batch = max_batch;
  c.max_frames = max_frames;
  c.max_tokens = max_tokens;
  int rc = workspaces_create(c);
  if (rc == JV_OK) return JV_OK;
  // Failure-atomic: a create that stopped part-way leaves workspace structs with null buffers behind.  Drop them and
  // come back at the capacities the caller had (they fitted before); if even that fails the context refuses every call.
  const std::string why = jv::g_last_error;
  (void)hipGetLastError();
  workspaces_destroy(c);
  c.max_batch = old_b;
  c.max_frames = old_f;
  c.max_tokens = old_t;
  if (workspaces_create(c) != JV_OK) {
    workspaces_destroy(c);
    c.broken = true;
    return jv::fail(rc, "jv_reserve: " + why + " -- and the previous capacities could not be restored: context unusable");
  }
  return jv::fail(rc, "jv_reserve: " + why + " (capacities unchanged)");
}

int jv_usable(const jv_context* ctx) { return ctx && !ctx->c.broken ? 1 : 0; }

void jv_destroy(jv_context* ctx) {
  if (!ctx) return;
  Context& c = ctx->c;
  (void)hipSetDevice(c.device);
  (void)hipDeviceSynchronize();
  workspaces_destroy(c);
  if (c.noise) (void)hipFree(c.noise);
  c.raw_arena.release();
  c.packed.release();
  jv::audio_ws_destroy(c);
  jv::resample_ws_destroy(c);
  jv::feat16k_ws_destroy(c);
  jv::align_ws_destroy(c);
  jv::level_ws_destroy(c);
  delete ctx;
}

int jv_num_tensors(const jv_context* ctx) { return ctx ? (int)ctx->c.raw.size() : 0; }
const char* jv_tensor_name(const jv_context* ctx, int i) {
  return (ctx && i >= 0 && i < (int)ctx->c.raw.size()) ? ctx->c.raw[i].name.c_str() : nullptr;
}
int jv_tensor_model(const jv_context* ctx, int i) {
  return (ctx && i >= 0 && i < (int)ctx->c.raw.size()) ? ctx->c.raw[i].model : -1;
}
int jv_tensor_ndim(const jv_context* ctx, int i) {
  return (ctx && i >= 0 && i < (int)ctx->c.raw.size()) ? (int)ctx->c.raw[i].shape.size() : -1;
}
int64_t jv_tensor_dim(const jv_context* ctx, int i, int d) {
  if (!ctx || i < 0 || i >= (int)ctx->c.raw.size()) return -1;
  const auto& s = ctx->c.raw[i].shape;
  return (d >= 0 && d < (int)s.size()) ? s[d] : -1;
}

int jv_load_tensor(jv_context* ctx, const char* name, const float* data, const int64_t* shape, int ndim, int on_device,
                   void* stream) {
  CTX_GUARD(ctx);
  if (!name || !data || !shape) return jv::fail(JV_ERR_ARG, "jv_load_tensor: null argument");
  Context& c = ctx->c;
  auto it = c.index.find(name);
  if (it == c.index.end()) return jv::fail(JV_ERR_NAME, std::string("unexpected key: ") + name);
  jv::RawTensor& t = c.raw[it->second];
  bool same = ndim == (int)t.shape.size();
  for (int d = 0; same && d < ndim; ++d) same = shape[d] == t.shape[d];
  if (!same) {
    std::string want, got;
    for (auto s : t.shape) want += std::to_string(s) + ",";
    for (int d = 0; d < ndim; ++d) got += std::to_string(shape[d]) + ",";
    return jv::fail(JV_ERR_SHAPE, std::string("size mismatch for ") + name + ": expected [" + want + "] got [" + got + "]");
  }
  if (c.ready[t.model] || (t.model == jv::MODEL_TTS && c.ready[jv::MODEL_FLOW] && jv::flow_part(t.name)))
    return jv::fail(JV_ERR_STATE, "model already finalized; create a new context to reload");
  if (!t.dev) JV_TRY(c.raw_arena.alloc((size_t)t.numel, &t.dev));
  hipStream_t st = static_cast<hipStream_t>(stream);
  JV_HIP(hipMemcpyAsync(t.dev, data, sizeof(float) * t.numel, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!on_device) JV_HIP(hipStreamSynchronize(st));
  t.loaded = true;
  return JV_OK;
}

int jv_load_noise(jv_context* ctx, const float* data, int64_t numel, int on_device, void* stream) {
  CTX_GUARD(ctx);
  if (!data || numel != (int64_t)jv::N_FEATS * jv::NOISE_FRAMES)
    return jv::fail(JV_ERR_SHAPE, "jv_load_noise: expected 80*15000 floats");
  hipStream_t st = static_cast<hipStream_t>(stream);
  JV_HIP(hipMemcpyAsync(ctx->c.noise, data, sizeof(float) * numel, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        st));
  if (!on_device) JV_HIP(hipStreamSynchronize(st));
  ctx->c.noise_loaded = true;
  return JV_OK;
}

int jv_finalize(jv_context* ctx, int model, void* stream) {
  CTX_GUARD(ctx);
  if (model != JV_MODEL_TTS && model != JV_MODEL_HIFT && model != JV_MODEL_PROMPT && model != JV_MODEL_FLOW)
    return jv::fail(JV_ERR_ARG, "jv_finalize: unknown model id");
  if (ctx->c.ready[model]) return JV_OK;
  if (model == JV_MODEL_TTS || model == JV_MODEL_FLOW) jv::flow_graphs_drop(ctx->c);
  return jv::finalize_model(ctx->c, model, static_cast<hipStream_t>(stream));
}

int jv_flow_estimator_step(jv_context* ctx, const float* x, const int32_t* lens, const float* mu, const float* t,
                           const float* spks, const float* cond, int B2, int T, float* out, void* stream) {
  CTX_GUARD(ctx);
  if (!x || !mu || !t || !spks || !cond || !out) return jv::fail(JV_ERR_ARG, "jv_flow_estimator_step: null tensor");
  return jv::flow_estimator(ctx->c, x, lens, mu, t, spks, cond, B2, T, out, static_cast<hipStream_t>(stream));
}

int jv_flow_estimator_masked(jv_context* ctx, const float* x, const float* mask, const float* mu, const float* t,
                             const float* spks, const float* cond, int B2, int T, float* out, void* stream) {
  CTX_GUARD(ctx);
  if (!x || !mask || !mu || !t || !spks || !cond || !out) return jv::fail(JV_ERR_ARG, "jv_flow_estimator_masked: null tensor");
  return jv::flow_estimator(ctx->c, x, nullptr, mu, t, spks, cond, B2, T, out, static_cast<hipStream_t>(stream), mask);
}

int jv_flow_estimator_tap(jv_context* ctx, int mode, const float* x, const int32_t* lens, const float* mu, const float* t,
                          const float* spks, const float* cond, int B, int T, int tap, float* out, int64_t out_floats, void* stream) {
  CTX_GUARD(ctx);
  if (!x || !mu || !t || !spks || !cond || !out) return jv::fail(JV_ERR_ARG, "jv_flow_estimator_tap: null tensor");
  return jv::flow_estimator_tap(ctx->c, mode, x, lens, mu, t, spks, cond, B, T, tap, out, (long)out_floats,
                                static_cast<hipStream_t>(stream));
}

int jv_flow_set_streaming(jv_context* ctx, int chunk_frames) {
  CTX_GUARD(ctx);
  if (chunk_frames < 0) return jv::fail(JV_ERR_ARG, "jv_flow_set_streaming: chunk must be >= 0");
  ctx->c.attn_chunk = chunk_frames;
  return JV_OK;
}

// (host state only: the rates reach the device with the next solve's schedule, so nothing in flight is touched)
int jv_flow_set_guidance(jv_context* ctx, const float* rates_host, int n) {
  CTX_GUARD(ctx);
  if (n < 0) return jv::fail(JV_ERR_ARG, "jv_flow_set_guidance: n must be >= 0");
  if (n > 0 && !rates_host) n = 0;
  for (int i = 0; i < n; ++i)
    if (!jv::guidance_rate_ok(rates_host[i])) {
      char msg[160];
      snprintf(msg, sizeof msg, "jv_flow_set_guidance: rate %d of %d is %g: a guidance rate must be finite and >= 0", i, n, (double)rates_host[i]);
      return jv::fail(JV_ERR_ARG, msg);
    }
  ctx->c.guidance.assign(rates_host, rates_host + n);
  return JV_OK;
}

// (host state only, like the guidance mode: the next solve's schedule and loop read it)
int jv_flow_set_solver(jv_context* ctx, int solver) {
  CTX_GUARD(ctx);
  if (solver != JV_SOLVER_EULER && solver != JV_SOLVER_MIDPOINT && solver != JV_SOLVER_HEUN) {
    char msg[160];
    snprintf(msg, sizeof msg, "jv_flow_set_solver: solver %d is none of JV_SOLVER_EULER, JV_SOLVER_MIDPOINT, JV_SOLVER_HEUN", solver);
    return jv::fail(JV_ERR_ARG, msg);
  }
  ctx->c.solver = solver;
  return JV_OK;
}

int jv_flow_set_graph(jv_context* ctx, int on) {
  CTX_GUARD(ctx);
  ctx->c.step_graphs = on != 0;
  if (!on && jv::flow_has_graphs(ctx->c)) {
    JV_HIP(hipDeviceSynchronize());      // a replay may still be executing on the private stream
    jv::flow_graphs_drop(ctx->c);
  }
  return JV_OK;
}

// A mode switch is a configuration call, not a hot-path one: it waits for everything this device has queued (solves on
// any stream, graph replays) before it touches the workspace, so nothing in flight sees half of each mode.
int jv_flow_set_contraction(jv_context* ctx, int exact_range) {
  CTX_GUARD(ctx);
  if (exact_range != 0 && ctx->c.est_fp16)
    return jv::fail(JV_ERR_STATE, "jv_flow_set_contraction: exact_range = 1 (bf16x6 everywhere) contradicts JV_PRECISION_FP16 "
                                  "(jv_flow_set_precision), which has nothing to drop from bf16x6; set the precision back first");
  if (ctx->c.exact_range != (exact_range != 0)) {
    JV_HIP(hipDeviceSynchronize());
    jv::flow_graphs_drop(ctx->c);                  // captured steps hold the old kernels
    jv::flow_ws_forget_attention(ctx->c, nullptr);   // that buffer holds fp32 rows in one mode, fp16 planes in the other
    JV_HIP(hipDeviceSynchronize());
  }
  ctx->c.exact_range = exact_range != 0;
  return JV_OK;
}

// (the planes keep their layout in both precisions: the attention buffer need not be forgotten)
int jv_flow_set_precision(jv_context* ctx, int precision) {
  CTX_GUARD(ctx);
  if (precision != JV_PRECISION_FP32 && precision != JV_PRECISION_FP16)
    return jv::fail(JV_ERR_ARG, "jv_flow_set_precision: JV_PRECISION_FP32 or JV_PRECISION_FP16");
  const bool fp16 = precision == JV_PRECISION_FP16;
  if (fp16 && ctx->c.exact_range)
    return jv::fail(JV_ERR_STATE, "jv_flow_set_precision: JV_PRECISION_FP16 contradicts exact_range = 1 (jv_flow_set_contraction: bf16x6 "
                                  "everywhere has no product to drop); set the contraction back first");
  if (ctx->c.est_fp16 != fp16) {
    JV_HIP(hipDeviceSynchronize());
    jv::flow_graphs_drop(ctx->c);      // captured steps hold the other mode's kernels
  }
  ctx->c.est_fp16 = fp16;
  return JV_OK;
}

int jv_flow_contraction_info(const jv_context* ctx, int32_t* out, int n) {
  if (!ctx || !out || n < 4) return jv::fail(JV_ERR_ARG, "jv_flow_contraction_info: null argument or fewer than 4 slots");
  if (!ctx->c.ready[jv::MODEL_FLOW]) return jv::fail(JV_ERR_STATE, "tts weights not finalized");
  int blocks = 0, all = 0, lin = 0, att = 0;
  for (int i = 0; i < jv::EST_NRES; ++i)
    for (int j = 0; j < jv::EST_NBLK; ++j) {
      const jv::BtbW& b = ctx->c.est.blk[i][j];
      ++blocks; lin += b.lin_h3; att += b.attn_h3; all += b.rows_ok;
    }
  out[0] = blocks; out[1] = all; out[2] = lin; out[3] = att;
  if (n >= 5) out[4] = ctx->c.est_fp16 ? JV_PRECISION_FP16 : JV_PRECISION_FP32;
  return JV_OK;
}

int jv_cfm_solve(jv_context* ctx, const float* mu, const int32_t* lens, const float* spks, const float* cond, int B, int T,
                 int n_timesteps, float temperature, const float* t_span_host, float* mel, void* stream) {
  CTX_GUARD(ctx);
  if (!mu || !spks || !cond || !mel) return jv::fail(JV_ERR_ARG, "jv_cfm_solve: null tensor");
  return jv::cfm_solve(ctx->c, mu, lens, spks, cond, B, T, n_timesteps, temperature, t_span_host, mel,
                       static_cast<hipStream_t>(stream));
}

int jv_cfm_solve_prompted(jv_context* ctx, const float* mu_y, const int32_t* y_lens, const float* prompt_h,
                          const float* prompt_feat, const int32_t* prompt_lens, const float* spks, int B, int Ty, int Ph, int Pf,
                          int n_timesteps, float temperature, const float* t_span_host, float* mel, void* stream) {
  CTX_GUARD(ctx);
  if (!mu_y || !y_lens || !prompt_lens || !spks || !mel) return jv::fail(JV_ERR_ARG, "jv_cfm_solve_prompted: null tensor");
  if ((Ph > 0 && !prompt_h) || (Pf > 0 && !prompt_feat)) return jv::fail(JV_ERR_ARG, "jv_cfm_solve_prompted: null prompt tensor");
  return jv::cfm_solve_prompted(ctx->c, mu_y, y_lens, prompt_h, prompt_feat, prompt_lens, spks, B, Ty, Ph, Pf, n_timesteps,
                                temperature, t_span_host, mel, static_cast<hipStream_t>(stream));
}

int jv_cfm_pool_admit(jv_context* ctx, const float* mu_y, const float* prompt_h, const float* prompt_feat, const float* spks,
                      const int32_t* y_lens_host, const int32_t* prompt_lens_host, const int32_t* slots_host,
                      const float* temperature_host, int B, int Ty, int Ph, int Pf, float* pool_x, float* pool_mu, float* pool_cond,
                      float* pool_spks, float* pool_amax, int slots, int Tcap, void* stream) {
  CTX_GUARD(ctx);
  if (!spks || !y_lens_host || !prompt_lens_host || !slots_host || !temperature_host || !pool_x || !pool_mu || !pool_cond ||
      !pool_spks || !pool_amax)
    return jv::fail(JV_ERR_ARG, "jv_cfm_pool_admit: null argument");
  if ((Ty > 0 && !mu_y) || (Ph > 0 && !prompt_h) || (Pf > 0 && !prompt_feat)) return jv::fail(JV_ERR_ARG, "jv_cfm_pool_admit: null tensor");
  return jv::cfm_pool_admit(ctx->c, mu_y, prompt_h, prompt_feat, spks, y_lens_host, prompt_lens_host, slots_host, temperature_host, B,
                            Ty, Ph, Pf, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, slots, Tcap, static_cast<hipStream_t>(stream));
}

int jv_cfm_pool_step(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                     float* pool_amax, int slots, int Tcap, const int32_t* slots_host, const int32_t* lens_host, const float* t_host,
                     const float* dt_host, int B, void* stream) {
  CTX_GUARD(ctx);
  if (!pool_x || !pool_mu || !pool_cond || !pool_spks || !pool_amax || !slots_host || !lens_host || !t_host || !dt_host)
    return jv::fail(JV_ERR_ARG, "jv_cfm_pool_step: null argument");
  return jv::cfm_pool_step(ctx->c, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, slots, Tcap, slots_host, lens_host, t_host,
                           dt_host, B, static_cast<hipStream_t>(stream));
}

int jv_cfm_pool_step_g(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                       float* pool_amax, int slots, int Tcap, const int32_t* slots_host, const int32_t* lens_host, const float* t_host,
                       const float* dt_host, const float* cfg_host, int B, void* stream) {
  CTX_GUARD(ctx);
  if (!pool_x || !pool_mu || !pool_cond || !pool_spks || !pool_amax || !slots_host || !lens_host || !t_host || !dt_host || !cfg_host)
    return jv::fail(JV_ERR_ARG, "jv_cfm_pool_step_g: null argument");
  return jv::cfm_pool_step(ctx->c, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, slots, Tcap, slots_host, lens_host, t_host,
                           dt_host, B, static_cast<hipStream_t>(stream), cfg_host);
}

int jv_cfm_pool_step_s(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                       float* pool_amax, float* pool_x0, float* pool_k1, int slots, int Tcap, const int32_t* slots_host,
                       const int32_t* lens_host, const float* t_host, const float* coef_host, const float* cfg_host,
                       const int32_t* stage_host, int B, void* stream) {
  CTX_GUARD(ctx);
  if (!pool_x || !pool_mu || !pool_cond || !pool_spks || !pool_amax || !slots_host || !lens_host || !t_host || !coef_host || !cfg_host ||
      !stage_host)
    return jv::fail(JV_ERR_ARG, "jv_cfm_pool_step_s: null argument");
  static_assert(JV_STAGE_EULER == jv::STAGE_EULER && JV_STAGE_MID1 == jv::STAGE_MID1 && JV_STAGE_MID2 == jv::STAGE_MID2 &&
                JV_STAGE_HEUN1 == jv::STAGE_HEUN1 && JV_STAGE_HEUN2 == jv::STAGE_HEUN2, "the header's stage codes are jv_ops.h's");
  return jv::cfm_pool_step(ctx->c, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, slots, Tcap, slots_host, lens_host, t_host,
                           coef_host, B, static_cast<hipStream_t>(stream), cfg_host, stage_host, pool_x0, pool_k1);
}

int jv_cfm_pool_fetch(jv_context* ctx, const float* pool_x, int slots, int Tcap, const int32_t* slots_host, const int32_t* first_host,
                      const int32_t* lens_host, int B, int Tm, float* mel, void* stream) {
  CTX_GUARD(ctx);
  if (!pool_x || !slots_host || !first_host || !lens_host || !mel) return jv::fail(JV_ERR_ARG, "jv_cfm_pool_fetch: null argument");
  return jv::cfm_pool_fetch(ctx->c, pool_x, slots, Tcap, slots_host, first_host, lens_host, B, Tm, mel,
                            static_cast<hipStream_t>(stream));
}

// ---- operator-level entry points -------------------------------------------------------------------
int jv_op_conv_gemm(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, int dil, const float* W, int N,
                    const float* bias, int act, int prologue, const float* alpha, float slope, const float* ln_g,
                    const float* ln_b, float ln_eps, const uint8_t* rowmask, const float* res, float* out, void* stream) {
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  jv::ConvGemmArgs a;
  jv::conv_gemm_defaults(a);
  a.A = A; a.lda = Cin; a.a_rows = a_rows; a.M = M; a.Cin = Cin; a.ntaps = ntaps; a.tap_row0 = tap_row0; a.tap_dil = dil;
  a.W = W; a.ldw = ntaps * Cin; a.n_rows_w = N; a.N = N; a.bias = bias; a.out = out; a.ldo = N;
  a.act = act; a.pro = prologue; a.pro_alpha = alpha; a.pro_slope = slope;
  if (ln_g) { a.ln = 1; a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps; }
  a.rowmask_in = rowmask; a.rowmask_out = rowmask;
  a.res1 = res; a.ldr1 = N;
  if (jv::dyn_env("JV_OP_X6")) {   // exercise the bf16x6 main loop: split W into three bf16 planes on the fly
    unsigned short* scratch = nullptr;
    const size_t n = (size_t)N * ntaps * Cin;
    JV_TRY(op_scratch(OPS_X6, 3 * n * sizeof(unsigned short) + 64, reinterpret_cast<void**>(&scratch)));
    JV_TRY(jv::split3_planes(W, scratch, (long)n, static_cast<hipStream_t>(stream)));
    a.W3 = scratch;
    a.w3_plane = (long)n;
  }
  return jv::conv_gemm(a, 1, static_cast<hipStream_t>(stream));
}

// products per fp16x3 step of the operator hooks below (jv_op_set_products): process-wide, never read by a context's calls
static int g_op_products = 3;
int jv_op_set_products(int np) {
  if (np != 1 && np != 3) return jv::fail(JV_ERR_ARG, "jv_op_set_products: 3 (fp16x3) or 1 (the hi x hi product alone)");
  g_op_products = np;
  return JV_OK;
}

// host logic of the fp16x3 scale choice (no device work): largest power of two s with bound * s <= 60000, 0 = unusable
float jv_h3_scale_for_bound(float bound) { return jv::h3_scale_for_bound(bound); }

// y = act(A W^T + bias) (+ res) through the fp16x3 main loop; a_bound: the caller's proven bound on |A| (test hook)
int jv_op_linear_h3(const float* A, int64_t rows, int M, int K, const float* W, int N, const float* bias, int act,
                    const float* res, float a_bound, int presplit, float* out, void* stream) {
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K % 32 || N <= 0 || M <= 0) return jv::fail(JV_ERR_ARG, "jv_op_linear_h3: K must be a multiple of 32");
  const float sc = jv::h3_scale_for_bound(a_bound);
  if (!(sc > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_linear_h3: unusable bound");
  void* scratch = nullptr;
  const size_t n = (size_t)N * K;
  const size_t need = n * 8 + (size_t)N * 12 + 512;
  JV_TRY(op_scratch(OPS_H3, need, &scratch));
  unsigned short* planes = static_cast<unsigned short*>(scratch);
  float* cs = reinterpret_cast<float*>(static_cast<char*>(scratch) + ((n * 4 + 63) & ~(size_t)63));
  JV_TRY(jv::split2h_planes(W, N, K, cs + N, planes, cs, st));
  jv::ConvGemmArgs a;
  jv::conv_gemm_defaults(a);
  a.A = A; a.lda = K; a.a_rows = rows; a.M = M; a.Cin = K; a.ntaps = 1; a.tap_row0 = 0; a.tap_dil = 1;
  a.W = W; a.ldw = K; a.n_rows_w = N; a.N = N; a.bias = bias; a.out = out; a.ldo = N; a.act = act;
  a.res1 = res; a.ldr1 = N;
  a.W2 = planes; a.w2_plane = (long)n; a.colscale = cs; a.a_scale = sc;
  if (presplit) {      // A as fp16 planes written by a producer kernel; 2 = reuse the planes of the previous call (timing)
    unsigned short* ap = nullptr;
    const size_t an = (size_t)rows * K;
    JV_TRY(op_scratch(OPS_H3_A, an * 4, reinterpret_cast<void**>(&ap)));
    if (presplit == 1) JV_TRY(jv::split2h_rows(A, K, ap, (long)an, rows, K, sc, st));
    a.A2 = ap; a.a2_plane = (long)an; a.lda2 = K;
  }
  a.np = g_op_products;
  return jv::conv_gemm(a, 1, st);
}

int jv_op_attention(const float* qkv, const int32_t* lens, int B, int G, int S, int L, float* out, void* stream) {
  jv::AttnArgs at{};
  at.qkv = qkv; at.ld = 1536; at.k_off = 512; at.v_off = 1024; at.out = out; at.ldo = 512;
  at.B = B; at.H = 8; at.G = G; at.S = S; at.L = L; at.lens = lens; at.chunk = 0;
  return jv::attention64(at, static_cast<hipStream_t>(stream));
}

// The conformer block's relative-position attention on caller-supplied buffers: relattn.hip's one launch (fused) or the block's
// three-GEMM sequence (prompt.hip rel_attention_gemm) with temporaries of this call (test hook)
int jv_op_rel_attention(const float* qkv, const float* p, const float* u, const float* v, const int64_t* lens, int B, int T, int G,
                        int S, int len_mul, int chunk, int fused, float* out, void* stream) {
  if (!qkv || !p || !u || !v || !lens || !out) return jv::fail(JV_ERR_ARG, "jv_op_rel_attention: null argument");
  if (B < 1 || T < 1 || G < 0 || S < T || len_mul < 1 || chunk < 0) return jv::fail(JV_ERR_ARG, "jv_op_rel_attention: bad geometry");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long* len = reinterpret_cast<const long*>(lens);
  if (fused) return jv::rel_attention(qkv, p, 2L * T - 1, u, v, len, len_mul, B, T, G, S, chunk, out, st);
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  const size_t rows = (size_t)G + (size_t)B * S, ld = (size_t)jv::round_up(T, 32), ldb = (size_t)jv::round_up(2 * T - 1, 32);
  const size_t n_q = rows * 512, n_ac = (size_t)B * 8 * T * ld, n_bd = (size_t)B * 8 * T * ldb, n_vt = (size_t)B * 8 * 64 * ld,
               n_p = (ldb + 128) * 512;      // (p with the zero rows behind 2T - 1 that the encoder's workspace has)
  float* tmp = nullptr;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(float) * (2 * n_q + n_ac + n_bd + n_vt + n_p)));
  float *qu = tmp, *qv = qu + n_q, *ac = qv + n_q, *bd = ac + n_ac, *vt = bd + n_bd, *pp = vt + n_vt;
  int rc = JV_OK;
  if (hipMemsetAsync(tmp, 0, sizeof(float) * (2 * n_q + n_ac + n_bd + n_vt + n_p), st) != hipSuccess ||
      hipMemcpyAsync(pp, p, sizeof(float) * (2 * (size_t)T - 1) * 512, hipMemcpyDeviceToDevice, st) != hipSuccess)
    rc = jv::fail(JV_ERR_HIP, "jv_op_rel_attention: staging failed");
  if (rc == JV_OK) rc = jv::rel_attention_gemm(qkv, pp, u, v, qu, qv, ac, bd, vt, out, len, len_mul, B, T, G, S, chunk, st);
  if (rc == JV_OK) rc = jv::zero_rows_behind(out, len, len_mul, B, T, G, S, st);
  const hipError_t se = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  if (rc == JV_OK && se != hipSuccess) rc = jv::fail(JV_ERR_HIP, std::string("jv_op_rel_attention: ") + hipGetErrorString(se));
  return rc;
}

// The text encoder's attention on caller-supplied buffers: encattn.hip's one launch (fused) or the layer's four-launch sequence
// (encoder.hip enc_attention_gemm) with temporaries of this call (test hook)
int jv_op_enc_attention(const float* qkv, const int64_t* lens, int B, int T, int G, int S, int fused, float* out, void* stream) {
  if (!qkv || !lens || !out) return jv::fail(JV_ERR_ARG, "jv_op_enc_attention: null argument");
  if (B < 1 || T < 1 || G < 0 || S < T) return jv::fail(JV_ERR_ARG, "jv_op_enc_attention: bad geometry");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long* len = reinterpret_cast<const long*>(lens);
  if (fused) return jv::enc_attention(qkv, len, B, T, G, S, out, st);
  if (T > jv::ENC_ATTN_GEMM_MAX) return jv::fail(JV_ERR_SHAPE, "jv_op_enc_attention: the four-launch route supports up to 512 tokens");
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  const size_t ld = (size_t)jv::round_up(T, 32), n_sc = (size_t)B * 2 * T * ld, n_vt = (size_t)B * 2 * 288 * ld;
  float* tmp = nullptr;
  JV_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(float) * (n_sc + n_vt)));
  int rc = JV_OK;
  if (hipMemsetAsync(tmp, 0, sizeof(float) * (n_sc + n_vt), st) != hipSuccess) rc = jv::fail(JV_ERR_HIP, "jv_op_enc_attention: staging failed");
  if (rc == JV_OK) rc = jv::enc_attention_gemm(qkv, tmp, tmp + n_sc, out, len, B, T, G, S, st);
  const hipError_t se = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  if (rc == JV_OK && se != hipSuccess) rc = jv::fail(JV_ERR_HIP, std::string("jv_op_enc_attention: ") + hipGetErrorString(se));
  return rc;
}

int jv_flow_token2mel(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                      const int64_t* token_lens, const float* prompt_feat, const int32_t* feat_lens, const float* embedding, int B,
                      int P, int N, int F, int streaming, int n_timesteps, float temperature, const float* t_span_host, float* mel,
                      int32_t* mel_lens, void* stream) {
  CTX_GUARD(ctx);
  if (!token_lens || !feat_lens || !embedding || !mel || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)) ||
      (F > 0 && !prompt_feat))
    return jv::fail(JV_ERR_ARG, "jv_flow_token2mel: null tensor");
  return jv::flow_token2mel(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                            reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), prompt_feat, feat_lens,
                            embedding, B, P, N, F, streaming, n_timesteps, temperature, t_span_host, mel, mel_lens,
                            static_cast<hipStream_t>(stream));
}

int jv_flow_token2mel_partial(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                              const int64_t* token_lens, const float* prompt_feat, const int32_t* feat_lens, const float* embedding,
                              int P, int N, int F, int streaming, int n_timesteps, float temperature, const float* t_span_host,
                              float* mel, int32_t* mel_lens, void* stream) {
  CTX_GUARD(ctx);
  if (!token_lens || !feat_lens || !embedding || !mel || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)) ||
      (F > 0 && !prompt_feat))
    return jv::fail(JV_ERR_ARG, "jv_flow_token2mel_partial: null tensor");
  return jv::flow_token2mel(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                            reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), prompt_feat, feat_lens,
                            embedding, 1, P, N, F, streaming, n_timesteps, temperature, t_span_host, mel, mel_lens,
                            static_cast<hipStream_t>(stream), 3);
}

int jv_flow_token2mel_ctx(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                          const int64_t* token_lens, const int32_t* ctx_lens, const float* prompt_feat, const int32_t* feat_lens,
                          const float* embedding, int B, int P, int N, int F, int streaming, int n_timesteps, float temperature,
                          const float* t_span_host, float* mel, int32_t* mel_lens, void* stream) {
  CTX_GUARD(ctx);
  if (!token_lens || !ctx_lens || !feat_lens || !embedding || !mel || (N > 0 && !tokens) ||
      (P > 0 && (!prompt_tokens || !prompt_lens)) || (F > 0 && !prompt_feat))
    return jv::fail(JV_ERR_ARG, "jv_flow_token2mel_ctx: null tensor");
  return jv::flow_token2mel(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                            reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), prompt_feat, feat_lens,
                            embedding, B, P, N, F, streaming, n_timesteps, temperature, t_span_host, mel, mel_lens,
                            static_cast<hipStream_t>(stream), 0, ctx_lens);
}

// conv_gemm through the fp16x3 main loop with a MEASURED bound: amax_in = device float >= max |A| (e.g. the amax_out of
// the launch that produced A), a_extra = what the prologue can add; amax_out (optional) receives max |out| (test hook)
int jv_op_conv_h3_measured(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, int dil, const float* W,
                           int N, const float* bias, int act, int prologue, const float* alpha, float slope,
                           const uint8_t* rowmask, const float* res, const float* amax_in, float a_extra, float* amax_out,
                           float* out, void* stream) {
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)N * ntaps * Cin;
  void* scratch = nullptr;
  const size_t need = n * 10 + (size_t)N * 12 + 512;      // 2 fp16 + 3 bf16 planes, colscale, row stats
  JV_TRY(op_scratch(OPS_CONV, need, &scratch));
  unsigned short* planes2 = static_cast<unsigned short*>(scratch);
  unsigned short* planes3 = planes2 + 2 * n;
  float* cs = reinterpret_cast<float*>(static_cast<char*>(scratch) + ((n * 10 + 63) & ~(size_t)63));
  jv::ConvGemmArgs a;
  jv::conv_gemm_defaults(a);
  a.A = A; a.lda = Cin; a.a_rows = a_rows; a.M = M; a.Cin = Cin; a.ntaps = ntaps; a.tap_row0 = tap_row0; a.tap_dil = dil;
  a.W = W; a.ldw = ntaps * Cin; a.n_rows_w = N; a.N = N; a.bias = bias; a.out = out; a.ldo = N;
  a.act = act; a.pro = prologue; a.pro_alpha = alpha; a.pro_slope = slope;
  a.rowmask_in = rowmask; a.rowmask_out = rowmask;
  a.res1 = res; a.ldr1 = N;
  a.amax_out = amax_out;
  if (amax_in) {
    JV_TRY(jv::split2h_planes(W, N, ntaps * Cin, cs + N, planes2, cs, st));
    a.W2 = planes2; a.w2_plane = (long)n; a.colscale = cs; a.amax_in = amax_in; a.a_extra = a_extra;
  } else {      // producer only: bf16x6
    JV_TRY(jv::split3_planes(W, planes3, (long)n, st));
    a.W3 = planes3; a.w3_plane = (long)n;
  }
  a.np = g_op_products;
  return jv::conv_gemm(a, 1, st);
}

// A contraction to 256 channels on the estimator's short-M route, from fp32 operands: conv_splitk (rowops.hip) -- the split-K tiles
// and splitk_reduce_rows' tail, the launcher Est::splitk calls -- with the weight planes and the partial sums in hook scratch.
// mode: how A and W are scaled, as the estimator's three kinds of split launches: 0 bf16x6 (the first resnet's block1), 1 fp16x3
// with the measured per-utterance bounds amax_in[slot_nb] (the other convolutions; slot(row) = clamp((row - slot_G) / slot_S), or
// slot_S < 0: row_sample[row]), 2 fp16x3 with the proven a_bound (to_out, ff.net.2).  rowmask serves as rowmask_in, rowmask_out and
// amax_mask (causal3 + ln_mish + track)
int jv_op_splitk(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, const float* W, int N, const float* bias,
                 const float* ln_g, const float* ln_b, int act, const uint8_t* rowmask, const float* rowvec,
                 const int32_t* row_sample, int rowvec_ld, const float* res, int64_t ldr, float* out, int64_t ldo, const float* ln2_g,
                 const float* ln2_b, float* out2, int ksplit_max, int mode, const float* amax_in, float a_bound, int slot_G,
                 int slot_S, int slot_nb, float* amax_out, void* stream) {
  static bool inited = false;
  if (!inited) {
    JV_TRY(jv::conv_gemm_init());
    inited = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N != 256) return jv::fail(JV_ERR_ARG, "jv_op_splitk: the split-K tail exists for N = 256 only");
  if (!A || !W || !out || M <= 0 || a_rows < M || Cin <= 0 || (Cin & 31) || ntaps < 1 || ksplit_max < 1 || ksplit_max > 64 ||
      mode < 0 || mode > 2 || (ldo & 3) || ldo < 256 || (res && ((ldr & 3) || ldr < 256)) || (rowvec_ld & 3) || rowvec_ld < 0)
    return jv::fail(JV_ERR_ARG, "jv_op_splitk: bad shape (Cin % 32, 1 <= ksplit_max <= 64, mode 0 .. 2, ldo / ldr / rowvec_ld % 4)");
  if ((ln_g != nullptr) != (ln_b != nullptr) || (ln2_g && (!ln2_b || !out2)))
    return jv::fail(JV_ERR_ARG, "jv_op_splitk: a LayerNorm needs gain and offset (and the second one out2)");
  if (!row_sample && ((rowvec && rowvec_ld) || (amax_out && slot_nb > 1) || (mode == 1 && slot_S < 0)))
    return jv::fail(JV_ERR_ARG, "jv_op_splitk: per-utterance vectors and slots need row_sample");
  if (mode == 1 && (!amax_in || slot_nb < 1)) return jv::fail(JV_ERR_ARG, "jv_op_splitk: mode 1 needs amax_in[slot_nb]");
  const float sc = mode == 2 ? jv::h3_scale_for_bound(a_bound) : 0.f;
  if (mode == 2 && !(sc > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_splitk: unusable bound");
  const size_t n = (size_t)N * ntaps * Cin;
  const int ksplit = ksplit_max < (Cin >> 5) ? ksplit_max : (Cin >> 5);      // conv_splitk's clamp: the partials it will write
  float* partial = nullptr;
  unsigned short* planes = nullptr;
  float *cs = nullptr, *stats = nullptr;
  auto layout = [&](Bump& b) {
    partial = b.take<float>((size_t)ksplit * M * 256);      // first: two calls at one M keep their partials at the same addresses
    planes = b.take<unsigned short>((mode == 0 ? 3 : 2) * n);
    cs = b.take<float>((size_t)N);
    stats = b.take<float>(2 * (size_t)N);
  };
  void* scratch = nullptr;
  { Bump b{nullptr}; layout(b); JV_TRY(op_scratch(OPS_SK, b.off, &scratch)); }
  { Bump b{static_cast<char*>(scratch)}; layout(b); }
  jv::ConvGemmArgs a;
  jv::conv_gemm_defaults(a);
  a.A = A; a.lda = Cin; a.a_rows = a_rows; a.M = M; a.Cin = Cin; a.ntaps = ntaps; a.tap_row0 = tap_row0; a.tap_dil = 1;
  a.W = W; a.ldw = ntaps * Cin; a.n_rows_w = N; a.N = N; a.bias = bias; a.out = out; a.ldo = ldo;
  if (ln_g) { a.ln = 1; a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = 1e-5f; }
  a.act = act;
  a.rowmask_in = rowmask; a.rowmask_out = rowmask;
  a.rowvec = rowvec; a.row_sample = row_sample; a.rowvec_ld = rowvec_ld;
  a.res1 = res; a.ldr1 = ldr;
  a.amax_out = amax_out; a.amax_mask = rowmask;
  if (mode == 0) {
    JV_TRY(jv::split3_planes(W, planes, (long)n, st));
    a.W3 = planes; a.w3_plane = (long)n;
  } else {
    JV_TRY(jv::split2h_planes(W, N, ntaps * Cin, stats, planes, cs, st));
    a.W2 = planes; a.w2_plane = (long)n; a.colscale = cs;
    if (mode == 2) {
      a.a_scale = sc;
    } else {
      a.amax_in = amax_in; a.a_extra = 0.f;
      a.amax_G = slot_G; a.amax_S = slot_S > 0 ? slot_S : 0; a.amax_nb = slot_nb; a.amax_rows = slot_S < 0 ? row_sample : nullptr;
    }
  }
  a.np = g_op_products;
  return jv::conv_splitk(a, ksplit_max, partial, row_sample, ln2_g, ln2_b, out2, st);
}

// the fp16x3 attention kernel; q_bound, k_bound, v_bound: the caller's proven bounds on |q|, |k|, |v| (test hook)
int jv_op_attention_h3(const float* qkv, const int32_t* lens, int B, int G, int S, int L, float q_bound, float k_bound,
                       float v_bound, float* out, void* stream) {
  jv::AttnArgs at{};
  at.qkv = qkv; at.ld = 1536; at.k_off = 512; at.v_off = 1024; at.out = out; at.ldo = 512;
  at.B = B; at.H = 8; at.G = G; at.S = S; at.L = L; at.lens = lens; at.chunk = 0;
  at.q_scale = jv::h3_scale_for_bound(q_bound * 0.1803369f);
  at.k_scale = jv::h3_scale_for_bound(k_bound);
  at.v_scale = jv::h3_scale_for_bound(v_bound);
  if (!(at.q_scale > 0.f && at.k_scale > 0.f && at.v_scale > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_attention_h3: unusable bound");
  at.np = g_op_products;
  return jv::attention64(at, static_cast<hipStream_t>(stream));
}

// the row-owning fp16x3 GEMM (rowgemm_kernel.h) with each of its epilogues (test / tuning hook): A [rows,K] fp32 is split
// into planes here (presplit = 2: reuse the planes of the previous call, timing only); epi: 0 plain, 1 GELU -> planes,
// 2 + res, 3 + res -> LayerNorm -> planes.  out: fp32 [M,N] (epi 0, 2, 3); out2: planes [2][M][N] (epi 1) / [2][M][256] (epi 3)
int jv_op_rowgemm(const float* A, int64_t rows, int M, int K, const float* W, int N, const float* bias, int epi,
                  const float* res, const float* ln_g, const float* ln_b, float a_bound, float out2_scale, int presplit,
                  float* out, uint16_t* out2, float* amax_out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float sc = jv::h3_scale_for_bound(a_bound);
  if (!(sc > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_rowgemm: unusable bound");
  void* scratch = nullptr;
  const size_t n = (size_t)N * K;
  const size_t need = n * 8 + (size_t)N * 12 + 512;
  JV_TRY(op_scratch(OPS_RG, need, &scratch));
  unsigned short* planes = static_cast<unsigned short*>(scratch);
  float* cs = reinterpret_cast<float*>(static_cast<char*>(scratch) + ((n * 4 + 63) & ~(size_t)63));
  JV_TRY(jv::split2h_planes(W, N, K, cs + N, planes, cs, st));
  unsigned short* wf = reinterpret_cast<unsigned short*>(static_cast<char*>(scratch) + ((n * 4 + (size_t)N * 12 + 511) & ~(size_t)255));
  if (!(K & 63)) JV_TRY(jv::pack_wfrag(planes, (long)n, K, N, K, wf, (long)n, st));
  unsigned short* ap = nullptr;
  const size_t an = (size_t)rows * K;
  JV_TRY(op_scratch(OPS_RG_A, an * 4, reinterpret_cast<void**>(&ap)));
  if (presplit != 2) JV_TRY(jv::split2h_rows(A, K, ap, (long)an, rows, K, sc, st));
  jv::RowGemmArgs a{};
  a.A2 = ap; a.a2_plane = (long)an; a.a_rows = rows; a.lda2 = K;
  a.M = M; a.K = K; a.N = N;
  a.W2 = planes; a.w2_plane = (long)n; a.ldw = K; a.colscale = cs; a.a_scale = sc; a.bias = bias;
  if (!(K & 63)) { a.Wf = wf; a.wf_plane = (long)n; }
  a.out = out; a.ldo = N; a.res = res; a.ldr = N;
  a.out2 = out2; a.out2_plane = (long)M * (epi == jv::RG_RES_LN ? 256 : N); a.ldo2 = epi == jv::RG_RES_LN ? 256 : N;
  a.out2_scale = out2_scale;
  a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = 1e-5f;
  a.amax_out = amax_out;
  a.np = g_op_products;
  return jv::rowgemm(a, epi, st);
}

// rowgemm's q | k | v epilogue (RG_QKV: rowgemm_wa_kernel with the column chunks dealt over nsplit workgroups per row tile, or
// rowgemm_wd_kernel): A [rows, K] fp32 split here with the scale of a_bound -- or A2, fp16 planes [2][rows][K] a producer wrote with
// that scale (rowres' / rowblock's LayerNorm1 planes) -- W [1536, K] (no bias); q -> fp32 [rows, 512], k | v -> planes [2][rows][1024]
// of k * scale(k_bound), v * scale(v_bound); rt: tile height 2 .. 5 (0: rowgemm_tile)
int jv_op_rowgemm_qkv(const float* A, const uint16_t* A2, int64_t rows, int M, int K, const float* W, float a_bound, float k_bound,
                      float v_bound, int nsplit, int rt, float* q, uint16_t* kv2, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float sc = jv::h3_scale_for_bound(a_bound), ks = jv::h3_scale_for_bound(k_bound), vs = jv::h3_scale_for_bound(v_bound);
  if (!(sc > 0.f && ks > 0.f && vs > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_rowgemm_qkv: unusable bound");
  if ((!A && !A2) || !W || !q || !kv2 || rows < M || M <= 0 || K <= 0 || (K & 63)) return jv::fail(JV_ERR_ARG, "jv_op_rowgemm_qkv: needs A or its planes, W, both outputs, rows >= M and K % 64 == 0");
  OpW w;
  void* scratch = nullptr;
  { Bump b{nullptr}; w.take(b, 1536, K, true); JV_TRY(op_scratch(OPS_QKV, b.off, &scratch)); }
  { Bump b{static_cast<char*>(scratch)}; w.take(b, 1536, K, true); }
  JV_TRY(w.pack(W, st, true));
  const unsigned short* ap = A2;
  if (!ap) {
    unsigned short* mine = nullptr;
    JV_TRY(op_scratch(OPS_QKV_A, (size_t)rows * K * 4, reinterpret_cast<void**>(&mine)));
    JV_TRY(jv::split2h_rows(A, K, mine, (long)rows * K, rows, K, sc, st));
    ap = mine;
  }
  jv::RowGemmArgs a{};
  a.A2 = ap; a.a2_plane = (long)rows * K; a.a_rows = rows; a.lda2 = K;
  a.M = M; a.K = K; a.N = 1536;
  a.W2 = w.planes; a.w2_plane = w.n(); a.ldw = K; a.colscale = w.cs; a.a_scale = sc;
  a.Wf = w.wf; a.wf_plane = w.n();
  a.ln_eps = 1e-5f;
  a.nsplit = nsplit; a.rt = rt;
  a.out = q; a.ldo = 512;
  a.out2 = kv2; a.out2_plane = (long)rows * 1024; a.ldo2 = 1024; a.out2_scale = ks; a.out2_scale2 = vs;
  a.np = g_op_products;
  return jv::rowgemm(a, jv::RG_QKV, st);
}

// rowres (rowres_kernel.h): a whole CausalResnetBlock1D in one launch, optionally with the following block's LayerNorm1 planes
// (lnf_out) or its q | k | v (Wq).  x [rows, Cin]; W1 [256, 3 Cin] / W2 [256, 768] tap-major, Wr [256, Cin]; block1 | res_conv go
// through the registry's concatenation; h2_bound as the registry computes it.  amax_in: per-utterance bounds of x, addressed by
// (slot_G, slot_S, slot_nb) or, slot_S < 0, by row_slot [rows]; lnf_bound / k_bound / v_bound: the caller's bounds behind the
// plane scales of the LayerNorm1 output, k and v
int jv_op_rowres(const float* x, int64_t rows, int M, int Cin, const uint8_t* rowmask, const float* amax_in, int slot_G, int slot_S,
                 int slot_nb, const int32_t* row_slot, const float* W1, const float* b1, const float* ln1_g, const float* ln1_b,
                 const float* Wr, const float* br, const float* temb, const float* W2, const float* b2, const float* ln2_g,
                 const float* ln2_b, const float* lnf_g, const float* lnf_b, float lnf_bound, uint16_t* lnf_out, const float* Wq,
                 float k_bound, float v_bound, float* q, uint16_t* kv2, float* amax_out, float* out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!x || !W1 || !Wr || !W2 || !ln1_g || !ln1_b || rows < M || M <= 0 || Cin < 64 || (Cin & 63))
    return jv::fail(JV_ERR_ARG, "jv_op_rowres: needs x, the three weight matrices, LayerNorm1, rows >= M and Cin % 64 == 0");
  OpW w1, wr, w2, wq;
  unsigned short* wf4 = nullptr;
  auto layout = [&](Bump& b) {
    w1.take(b, 256, 3 * Cin, false);
    wr.take(b, 256, Cin, false);
    wf4 = b.take<unsigned short>(2 * 256 * 4 * (size_t)Cin);
    w2.take(b, 256, 768, true);
    if (Wq) wq.take(b, 1536, 256, true);
  };
  void* scratch = nullptr;
  { Bump b{nullptr}; layout(b); JV_TRY(op_scratch(OPS_RR, b.off, &scratch)); }
  { Bump b{static_cast<char*>(scratch)}; layout(b); }
  JV_TRY(w1.pack(W1, st, false));
  JV_TRY(wr.pack(Wr, st, false));
  JV_TRY(jv::pack_wfrag_res4(w1.planes, w1.n(), wr.planes, wr.n(), Cin, wf4, st));
  JV_TRY(w2.pack(W2, st, true));
  if (Wq) JV_TRY(wq.pack(Wq, st, true));
  float gm = 0.f, bm = 0.f;
  JV_TRY(jv::dev_maxabs(ln1_g, 256, 1, st, &gm));
  JV_TRY(jv::dev_maxabs(ln1_b, 256, 1, st, &bm));
  jv::RowResArgs a{};
  a.A = x; a.lda = Cin; a.a_rows = rows; a.M = M; a.Cin = Cin; a.rowmask = rowmask;
  a.amax_in = amax_in; a.slot_G = slot_G; a.slot_S = slot_S; a.slot_nb = slot_nb; a.row_slot = row_slot;
  a.Wf1 = wf4; a.wf1_plane = 256L * 4 * Cin;
  a.cs1 = w1.cs; a.b1 = b1; a.ln1_g = ln1_g; a.ln1_b = ln1_b;
  a.csr = wr.cs; a.br = br;
  a.temb = temb; a.h2_bound = jv::resnet_h2_bound(gm, bm); a.ln_eps = 1e-5f;
  a.Wf2 = w2.wf; a.wf2_plane = w2.n();
  a.cs2 = w2.cs; a.b2 = b2; a.ln2_g = ln2_g; a.ln2_b = ln2_b;
  a.out = out; a.ldo = 256; a.amax_out = amax_out;
  if (lnf_g) {
    a.lnf_g = lnf_g; a.lnf_b = lnf_b; a.lnf_scale = jv::h3_scale_for_bound(lnf_bound);
    if (!Wq) {
      a.lnf_out = lnf_out; a.lnf_plane = (long)rows * 256;
    } else {
      a.Wqf = wq.wf; a.wqf_plane = wq.n(); a.csq = wq.cs;
      a.q = q; a.kv2 = kv2; a.kv2_plane = (long)rows * 1024;
      a.k_scale = jv::h3_scale_for_bound(k_bound); a.v_scale = jv::h3_scale_for_bound(v_bound);
    }
  } else if (Wq || lnf_out) {
    return jv::fail(JV_ERR_ARG, "jv_op_rowres: the following block's planes and q | k | v need its LayerNorm1");
  }
  a.np = g_op_products;
  return jv::rowres(a, st);
}

// hiftpair (hiftpair_kernel.h): a vocoder ResBlock's two convolutions in one launch, out = ((Conv1d_k(Snake2(Conv1d_k,dil(Snake1(A)) + b1))
// + b2) + A + res2) * out_scale (+ out when accumulate); C = 64 / 128, ntaps = 3 / 7 / 11; W1, W2 [C][ntaps * C] tap-major, packed as
// one fragment stream by the registry's concatenation; l1max, b1max, e1, e2 derived as at load time.  amax_in: per-utterance
// bounds of A, addressed by (slot_G, slot_S, slot_nb) or by slot_map [rows]
int jv_op_hiftpair(const float* A, int64_t rows, int C, int ntaps, int dil, const float* W1, const float* b1, const float* alpha1,
                   const float* W2, const float* b2, const float* alpha2, const uint8_t* rowmask, const float* amax_in, int slot_G,
                   int slot_S, int slot_nb, const int32_t* slot_map, const float* res2, float out_scale, int accumulate,
                   float* amax_out, float* out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!A || !W1 || !W2 || !alpha1 || !alpha2 || rows <= 0 || (C != 64 && C != 128) || ntaps < 1)
    return jv::fail(JV_ERR_ARG, "jv_op_hiftpair: needs A, both weight matrices and Snake alphas, 64 or 128 channels");
  const int K = ntaps * C;
  OpW w1, w2;
  unsigned short* wfp = nullptr;
  auto layout = [&](Bump& b) {
    w1.take(b, C, K, false);
    w2.take(b, C, K, false);
    wfp = b.take<unsigned short>(2 * (size_t)C * 2 * K);
  };
  void* scratch = nullptr;
  { Bump b{nullptr}; layout(b); JV_TRY(op_scratch(OPS_HP, b.off, &scratch)); }
  { Bump b{static_cast<char*>(scratch)}; layout(b); }
  JV_TRY(w1.pack(W1, st, false));
  JV_TRY(w2.pack(W2, st, false));
  JV_TRY(jv::pack_wfrag_pair(w1.planes, w1.n(), w2.planes, w2.n(), C, K, wfp, st));
  jv::HiftPairArgs a{};
  JV_TRY(jv::snake_extra_of(alpha1, C, st, &a.e1));
  JV_TRY(jv::snake_extra_of(alpha2, C, st, &a.e2));
  JV_TRY(jv::dev_maxabs(w1.stats + C, C, 1, st, &a.l1max));      // (row L1 norms: split2h_planes' second statistic)
  if (b1) JV_TRY(jv::dev_maxabs(b1, C, 1, st, &a.b1max));
  if (!(a.l1max > 0.f && a.l1max < 1e30f) || !(a.b1max == a.b1max && a.b1max < 1e30f))
    return jv::fail(JV_ERR_ARG, "jv_op_hiftpair: the first convolution's weights give no usable bound");
  a.A = A; a.a_rows = rows; a.M = (int)rows; a.ntaps = ntaps; a.dil = dil; a.rowmask = rowmask;
  a.alpha1 = alpha1; a.alpha2 = alpha2;
  a.Wf = wfp; a.wf_plane = (long)C * 2 * K;
  a.cs1 = w1.cs; a.b1 = b1; a.cs2 = w2.cs; a.b2 = b2;
  a.amax_in = amax_in; a.slot_G = slot_G; a.slot_S = slot_S; a.slot_nb = slot_nb; a.slot_map = slot_map;
  a.out = out; a.res2 = res2; a.out_scale = out_scale; a.accumulate = accumulate;
  a.amax_out = amax_out;
  return jv::hiftpair(a, C, st);
}

// The tail of a transformer block and the head of the next one (rowblock_kernel.h) from fp32 operands, as the estimator launches it:
//   mode 0  h += to_out(att); out = h + ff.net.2(gelu(ff.net.0(LayerNorm3(h))))
//   mode 1  ... and LayerNorm1_next(out) as planes [2][rows][256] to ln_out
//   mode 2  ... and q | k | v = Wq LayerNorm1_next(out): q fp32 [rows, 512], kv2 planes [2][rows][1024]
//   mode 3  the feed-forward alone (rowffn): `att` is x [rows, 256], the LayerNorm3 output, h the residual; ln1_g != NULL: planes to ln_out
// att [rows, 512] (modes 0 - 2), h [rows, 256] (in place: h after phase A), out = h or a separate buffer with its own ldo.
// fused = 1: one launch; 0: the separate launchers of JV_NO_BLOCK_FUSE on the same plane buffers (rowgemm<res,ln>, rowffn,
// rowgemm<qkv>); -1: those of JV_NO_FFN_FUSE as well (rowgemm<gelu> + rowgemm<res[,ln]> for the feed-forward).  *_bound: the caller's
// bounds behind the operand scales (att, LayerNorm3 output, hidden, LayerNorm1 output, k, v).  Row buffers must hold whole tiles.
int jv_op_rowblock(const float* att, float* h, int64_t rows, int M, int mode, int fused, float att_bound, const float* Wo,
                   const float* bo, const float* ln3_g, const float* ln3_b, float ln3_bound, const float* W1, const float* b1,
                   float hid_bound, const float* W2, const float* b2, const float* ln1_g, const float* ln1_b, float ln1_bound,
                   const float* Wq, float k_bound, float v_bound, float* out, int64_t ldo, uint16_t* ln_out, float* q, uint16_t* kv2,
                   float* amax_h, float* amax_out, const int32_t* row_slot, const uint8_t* row_mask, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode < 0 || mode > 3 || fused < -1 || fused > 1) return jv::fail(JV_ERR_ARG, "jv_op_rowblock: mode 0 .. 3, fused -1 .. 1");
  const bool ffn_only = mode == 3, qkv = mode == 2;
  const bool follows = mode == 1 || mode == 2 || (ffn_only && ln1_g);
  if (!att || !h || !out || !W1 || !W2 || rows < M || M <= 0 || (!ffn_only && (!Wo || !ln3_g || !ln3_b)) ||
      (follows && (!ln1_g || !ln1_b)) || (qkv && (!Wq || !q || !kv2)) || ((mode == 1 || (ffn_only && follows)) && !ln_out))
    return jv::fail(JV_ERR_ARG, "jv_op_rowblock: missing operand for this mode");
  const float sc_o = ffn_only ? 1.f : jv::h3_scale_for_bound(att_bound), sc_1 = jv::h3_scale_for_bound(ln3_bound);
  const float sc_h = jv::h3_scale_for_bound(hid_bound), sc_q = follows ? jv::h3_scale_for_bound(ln1_bound) : 1.f;
  const float sc_k = qkv ? jv::h3_scale_for_bound(k_bound) : 1.f, sc_v = qkv ? jv::h3_scale_for_bound(v_bound) : 1.f;
  if (!(sc_o > 0.f && sc_1 > 0.f && sc_h > 0.f && sc_q > 0.f && sc_k > 0.f && sc_v > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_rowblock: unusable bound");
  // the plane buffers of this hook hold whole tiles of the tallest tile height (80 rows); the caller's row buffers are checked by rowblock()
  const long R = ((long)rows + 79) / 80 * 80;
  OpW wo, w1, w2, wq;
  unsigned short *ap = nullptr, *lnp = nullptr, *ffp = nullptr;
  auto layout = [&](Bump& b) {
    if (!ffn_only) wo.take(b, 256, 512, true);
    w1.take(b, 1024, 256, true);
    w2.take(b, 256, 1024, true);
    if (qkv) wq.take(b, 1536, 256, true);
    ap = b.take<unsigned short>(2 * (size_t)R * (ffn_only ? 256 : 512));      // att planes (mode 3: the LayerNorm3 planes)
    lnp = b.take<unsigned short>(2 * (size_t)R * 256);                          // unfused: LayerNorm planes between the launches
    ffp = fused == -1 ? b.take<unsigned short>(2 * (size_t)R * 1024) : nullptr; // unfused feed-forward: the hidden planes
  };
  void* scratch = nullptr;
  { Bump b{nullptr}; layout(b); JV_TRY(op_scratch(OPS_RB, b.off, &scratch)); }
  { Bump b{static_cast<char*>(scratch)}; layout(b); }
  if (!ffn_only) JV_TRY(wo.pack(Wo, st, true));
  JV_TRY(w1.pack(W1, st, true));
  JV_TRY(w2.pack(W2, st, true));
  if (qkv) JV_TRY(wq.pack(Wq, st, true));
  const int KA = ffn_only ? 256 : 512;
  JV_HIP(hipMemsetAsync(ap, 0, 2 * (size_t)R * KA * sizeof(unsigned short), st));
  JV_TRY(jv::split2h_rows(att, KA, ap, R * KA, rows, KA, ffn_only ? sc_1 : sc_o, st));

  auto rg_args = [&](const unsigned short* planes, int K, const OpW& m, float a_scale, const float* bias) {
    jv::RowGemmArgs a{};
    a.A2 = planes; a.a2_plane = R * K; a.a_rows = rows; a.lda2 = K;
    a.M = M; a.K = K; a.N = m.N;
    a.W2 = m.planes; a.w2_plane = m.n(); a.ldw = K; a.colscale = m.cs; a.a_scale = a_scale;
    a.Wf = m.wf; a.wf_plane = m.n();
    a.bias = bias; a.ln_eps = 1e-5f; a.out2_scale = 1.f;
    a.np = g_op_products;
    return a;
  };
  // the feed-forward (+ the next LayerNorm1) from the LayerNorm3 planes `xin`, as one launch or two (estimator.hip: block_rows)
  auto feed_forward = [&](const unsigned short* xin, unsigned short* ln_dst) -> int {
    if (fused >= 0) {
      jv::RowFfnArgs f{};
      f.np = g_op_products;
      f.A2 = xin; f.a2_plane = R * 256; f.a_rows = rows; f.lda2 = 256; f.M = M;
      f.W1f = w1.wf; f.w1f_plane = w1.n(); f.cs1 = w1.cs; f.b1 = b1; f.a_scale1 = sc_1;
      f.h_scale = sc_h;
      f.W2f = w2.wf; f.w2f_plane = w2.n(); f.cs2 = w2.cs; f.b2 = b2;
      f.out = out; f.ldo = ldo; f.res = h; f.ldr = 256;
      f.ln_eps = 1e-5f; f.out2_scale = 1.f;
      f.amax_out = amax_out; f.row_slot = row_slot; f.row_mask = row_mask;
      if (follows) {
        f.ln = 1; f.out2 = ln_dst; f.out2_plane = ln_dst == lnp ? R * 256 : (long)rows * 256; f.ldo2 = 256; f.out2_scale = sc_q;
        f.ln_g = ln1_g; f.ln_b = ln1_b;
      }
      return jv::rowffn(f, st);
    }
    jv::RowGemmArgs a = rg_args(xin, 256, w1, sc_1, b1);
    a.out2 = ffp; a.out2_plane = R * 1024; a.ldo2 = 1024; a.out2_scale = sc_h;
    JV_TRY(jv::rowgemm(a, jv::RG_GELU_PL, st));
    a = rg_args(ffp, 1024, w2, sc_h, b2);
    a.out = out; a.ldo = ldo; a.res = h; a.ldr = 256;
    a.amax_out = amax_out; a.row_slot = row_slot; a.row_mask = row_mask;
    if (follows) {
      a.out2 = ln_dst; a.out2_plane = ln_dst == lnp ? R * 256 : (long)rows * 256; a.ldo2 = 256; a.out2_scale = sc_q;
      a.ln_g = ln1_g; a.ln_b = ln1_b;
      return jv::rowgemm(a, jv::RG_RES_LN, st);
    }
    return jv::rowgemm(a, jv::RG_RES, st);
  };
  if (ffn_only) return feed_forward(ap, follows ? ln_out : nullptr);

  if (fused == 1) {
    jv::RowBlockArgs f{};
    f.np = g_op_products;
    f.A2 = ap; f.a2_plane = R * 512; f.a_rows = rows; f.M = M;
    f.Wof = wo.wf; f.wof_plane = wo.n(); f.cso = wo.cs; f.bo = bo; f.a_scale_o = sc_o;
    f.h = h; f.ln3_g = ln3_g; f.ln3_b = ln3_b;
    f.W1f = w1.wf; f.w1f_plane = w1.n(); f.cs1 = w1.cs; f.b1 = b1; f.a_scale1 = sc_1;
    f.h_scale = sc_h;
    f.W2f = w2.wf; f.w2f_plane = w2.n(); f.cs2 = w2.cs; f.b2 = b2;
    f.out = out; f.ldo = ldo;
    f.amax_h = amax_h; f.amax_out = amax_out; f.row_slot = row_slot; f.row_mask = row_mask;
    if (follows) { f.ln1_g = ln1_g; f.ln1_b = ln1_b; f.a_scale_q = sc_q; }
    if (qkv) {
      f.Wqf = wq.wf; f.wqf_plane = wq.n(); f.csq = wq.cs;
      f.q = q; f.kv2 = kv2; f.kv2_plane = (long)rows * 1024; f.k_scale = sc_k; f.v_scale = sc_v;
    } else if (follows) {
      f.ln_out = ln_out; f.ln_out_plane = (long)rows * 256;
    }
    return jv::rowblock(f, qkv, st);
  }
  // the same rows through the separate launchers (the kernels the fused launch is built from)
  jv::RowGemmArgs a = rg_args(ap, 512, wo, sc_o, bo);      // h += to_out(att); ln = LayerNorm3(h)
  a.out = h; a.ldo = 256; a.res = h; a.ldr = 256;
  a.out2 = lnp; a.out2_plane = R * 256; a.ldo2 = 256; a.out2_scale = sc_1;
  a.ln_g = ln3_g; a.ln_b = ln3_b;
  a.amax_out = amax_h; a.row_slot = row_slot; a.row_mask = row_mask;
  JV_TRY(jv::rowgemm(a, jv::RG_RES_LN, st));
  JV_TRY(feed_forward(lnp, qkv ? lnp : ln_out));
  if (!qkv) return JV_OK;
  a = rg_args(lnp, 256, wq, sc_q, nullptr);
  a.out = q; a.ldo = 512;
  a.out2 = kv2; a.out2_plane = (long)rows * 1024; a.ldo2 = 1024; a.out2_scale = sc_k; a.out2_scale2 = sc_v;
  return jv::rowgemm(a, jv::RG_QKV, st);
}

// the row-owning causal k = 3 convolution (rowconv_kernel.h) with its fused row-wise tail (test / tuning hook): one
// measured-bound slot (amax_in, a device float >= max |A|), W [256, 3 Cin] packed tap-major like jv_op_conv_gemm
int jv_op_rowconv(const float* A, int64_t rows, int M, int Cin, const float* W, const float* bias, const float* ln_g,
                  const float* ln_b, int act, const uint8_t* rowmask, const float* rowvec, const float* res,
                  const float* amax_in, float* amax_out, float* out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = 256, K = 3 * Cin;
  void* scratch = nullptr;
  const size_t n = (size_t)N * K;
  const size_t head = ((n * 4 + (size_t)N * 12 + 256 + (size_t)rows * sizeof(int)) + 255) & ~(size_t)255;
  const size_t need = head + n * 4;      // + the planes again in fragment order
  JV_TRY(op_scratch(OPS_RC, need, &scratch));
  unsigned short* planes = static_cast<unsigned short*>(scratch);
  float* cs = reinterpret_cast<float*>(static_cast<char*>(scratch) + ((n * 4 + 63) & ~(size_t)63));
  int* slots = reinterpret_cast<int*>(cs + 3 * N + 16);
  unsigned short* wf = reinterpret_cast<unsigned short*>(static_cast<char*>(scratch) + head);
  JV_TRY(jv::split2h_planes(W, N, K, cs + N, planes, cs, st));
  const bool frag = !((Cin >> 5) & 1) && !(Cin & 31);
  if (frag) JV_TRY(jv::pack_wfrag(planes, (long)n, K, N, K, wf, (long)n, st));
  JV_HIP(hipMemsetAsync(slots, 0, (size_t)rows * sizeof(int), st));
  jv::RowConvArgs a{};
  a.A = A; a.lda = Cin; a.a_rows = rows; a.M = M; a.Cin = Cin; a.rowmask_in = rowmask;
  a.W2 = planes; a.w2_plane = (long)n; a.ldw = K; a.colscale = cs; a.amax_in = amax_in; a.row_slot = slots; a.bias = bias;
  if (frag) { a.Wf = wf; a.wf_plane = (long)n; }
  a.out = out; a.ldo = N;
  if (ln_g) { a.ln = 1; a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = 1e-5f; }
  a.act = act; a.rowmask_out = rowmask; a.rowvec = rowvec; a.rowvec_ld = N; a.res = res; a.ldr = N;
  a.amax_out = amax_out; a.row_mask = rowmask;
  a.np = g_op_products;
  return jv::rowconv(a, st);
}

// hiftconv (hiftconv_kernel.h): out = ((Conv1d_k,dil(Snake_alpha(A)) + bias) + res1 + res2) * out_scale (+ out when accumulate) on a
// [rows, C] row buffer, C = 64 / 128 / 256; W [C][ntaps * C] tap-major; amax_in / amax_out: slot_nb per-utterance slots, addressed
// by (slot_G, slot_S, slot_nb) or by slot_map [rows] as in jv_op_hiftpair; (0, 0, 1, NULL) is one slot for every row (test hook)
int jv_op_hiftconv(const float* A, int64_t rows, int C, int ntaps, int dil, const float* W, const float* bias, const float* alpha,
                   const uint8_t* rowmask, const float* res1, const float* res2, float out_scale, int accumulate,
                   const float* amax_in, float a_extra, int slot_G, int slot_S, int slot_nb, const int32_t* slot_map,
                   float* amax_out, float* out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (slot_nb < 1) return jv::fail(JV_ERR_ARG, "jv_op_hiftconv: needs at least one utterance slot");
  const int K = ntaps * C;
  void* scratch = nullptr;
  const size_t n = (size_t)C * K;
  const size_t head = ((n * 4 + (size_t)C * 12 + 256) + 255) & ~(size_t)255;
  const size_t need = head + n * 4;
  JV_TRY(op_scratch(OPS_HIFT, need, &scratch));
  unsigned short* planes = static_cast<unsigned short*>(scratch);
  float* cs = reinterpret_cast<float*>(static_cast<char*>(scratch) + ((n * 4 + 63) & ~(size_t)63));
  unsigned short* wf = reinterpret_cast<unsigned short*>(static_cast<char*>(scratch) + head);
  JV_TRY(jv::split2h_planes(W, C, K, cs + C, planes, cs, st));
  JV_TRY(jv::pack_wfrag(planes, (long)n, K, C, K, wf, (long)n, st));
  jv::HiftConvArgs a{};
  a.A = A; a.a_rows = rows; a.M = (int)rows; a.ntaps = ntaps; a.dil = dil; a.tap_row0 = -(dil * (ntaps - 1) / 2); a.rowmask_in = rowmask;
  a.alpha = alpha; a.Wf = wf; a.wf_plane = (long)n; a.colscale = cs; a.bias = bias;
  a.amax_in = amax_in; a.a_extra = a_extra; a.slot_G = slot_G; a.slot_S = slot_S; a.slot_nb = slot_nb; a.slot_map = slot_map;
  a.out = out; a.res1 = res1; a.res2 = res2; a.out_scale = out_scale; a.accumulate = accumulate;
  a.amax_out = amax_out; a.amax_mask = rowmask;
  return jv::hiftconv(a, C, st);
}

int jv_hift_lds_bytes(int pair, int C, int NG, int ntaps, int dil) { return jv::hift_lds_bytes(pair, C, NG, ntaps, dil); }

// attention64_planes (attention_pl.hip) on an fp32 qkv matrix: K and V are split into planes here the way the qkv GEMM's
// epilogue writes them; planes_out = 1: the result as fp16 planes [2][rows][512] of value * out2_scale (test hook)
int jv_op_attention_planes(const float* qkv, int64_t rows, const int32_t* lens, int B, int G, int S, int L, float q_bound,
                           float k_bound, float v_bound, int chunk, float out2_scale, float* out, uint16_t* out2, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned short* kv = nullptr;
  JV_TRY(op_scratch(OPS_ATTN, (size_t)rows * 1024 * 2 * sizeof(unsigned short), reinterpret_cast<void**>(&kv)));
  jv::AttnArgs at{};
  at.qkv = qkv; at.ld = 1536; at.out = out; at.ldo = 512;
  at.B = B; at.H = 8; at.G = G; at.S = S; at.L = L; at.lens = lens; at.chunk = chunk;
  at.q_scale = jv::h3_scale_for_bound(q_bound * 0.1803369f);
  at.k_scale = jv::h3_scale_for_bound(k_bound);
  at.v_scale = jv::h3_scale_for_bound(v_bound);
  if (!(at.q_scale > 0.f && at.k_scale > 0.f && at.v_scale > 0.f)) return jv::fail(JV_ERR_ARG, "jv_op_attention_planes: unusable bound");
  const long plane = (long)rows * 1024;
  JV_TRY(jv::split2h_rows(qkv + 512, 1536, kv, plane, rows, 512, at.k_scale, st, 1024));
  JV_TRY(jv::split2h_rows(qkv + 1024, 1536, kv + 512, plane, rows, 512, at.v_scale, st, 1024));
  at.kv2 = kv; at.kv2_plane = plane; at.kv_ld = 1024;
  if (out2) { at.out2 = out2; at.out2_plane = (long)rows * 512; at.out2_scale = out2_scale; }
  at.np = g_op_products;
  if (at.np == 1 && chunk == 0 && (jv::dyn_env("JV_OP_ATTN_ROWS") || jv::dyn_env("JV_OP_ATTN_SINGLE")))
    return jv::fail(JV_ERR_STATE, "jv_op_attention_planes: attention_r / attention_s have no one-product form");
  if (chunk == 0 && jv::dyn_env("JV_OP_ATTN_ROWS")) return jv::attention64_rows(at, st);      // the row-owning form (attention_r.hip)
  if (chunk == 0 && jv::dyn_env("JV_OP_ATTN_SINGLE")) return jv::attention64_single(at, st);  // one wave per SIMD (attention_s.hip)
  return jv::attention64_planes(at, st);
}

int jv_op_layernorm(const float* x, const float* g, const float* b, float eps, int64_t rows, int C, float* out, void* stream) {
  return jv::layernorm_rows(x, nullptr, out, g, b, eps, rows, C, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
