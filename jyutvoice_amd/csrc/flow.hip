// Flow-matching decoder: the workspace, the three entry points and the Euler / classifier-free-guidance solver
// (jyutvoice/flow/flow_matching.py:215-265, 356-401) around the estimator evaluation of estimator.hip.
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/jyutvoice_hip.h"
#include "flow_ws.h"

namespace jv {

static long flow_rows(int B2, int T) { return (long)FLOW_G + (long)B2 * (T + FLOW_GAP); }

int flow_ws_create(Context& c) {
  FlowWs* w = new FlowWs();
  c.flow = w;
  const int B2 = 2 * c.max_batch;
  // row indices are ints inside the kernels
  if (c.max_batch > (1 << 20) || flow_rows(B2, c.max_frames) > (1L << 30)) return fail(JV_ERR_SHAPE, "flow workspace: batch x frames beyond 2^30 rows");
  w->rows_alloc = round_up((int)flow_rows(B2, c.max_frames), 128) + 256;
  const size_t R = (size_t)w->rows_alloc;
  auto F = [&](float** p, size_t floats) { return ws_alloc(c, floats * sizeof(float), reinterpret_cast<void**>(p)); };
  JV_TRY(F(&w->x, R * 80));
  JV_TRY(F(&w->mu, R * 80));
  JV_TRY(F(&w->cond, R * 80));
  JV_TRY(F(&w->x0, R * 80));
  JV_TRY(F(&w->k1, R * 80));
  JV_TRY(F(&w->spks, (size_t)B2 * 80));
  JV_TRY(F(&w->xin, R * 320));
  JV_TRY(F(&w->h, R * 256));
  JV_TRY(F(&w->h2, R * 256));
  JV_TRY(F(&w->res, R * 256));
  JV_TRY(F(&w->cat, R * 512));
  JV_TRY(F(&w->ln, R * 256));
  JV_TRY(F(&w->qkv, R * 1536));
  JV_TRY(F(&w->att, R * 512));
  JV_TRY(F(&w->ff, R * 1024));
  JV_TRY(F(&w->d, R * 80));
  JV_TRY(F(&w->partial, (size_t)PARTIAL_SPLITS * PARTIAL_ROWS * 256));
  JV_TRY(F(&w->tsin, (size_t)B2 * 320));
  JV_TRY(F(&w->t1, (size_t)B2 * 1024));
  JV_TRY(F(&w->tmish, (size_t)B2 * 1024));
  JV_TRY(F(&w->temb, (size_t)B2 * EST_NRES * 256));
  JV_TRY(F(&w->tfreq, 160));
  {
    float freq[160];
    time_freq_table(freq);
    JV_HIP(hipMemcpy(w->tfreq, freq, sizeof(freq), hipMemcpyHostToDevice));
  }
  w->amax_stride = B2;
  JV_TRY(F(&w->amax, (size_t)3 * B2));
  JV_TRY(F(&w->t_dev, (size_t)B2));
  JV_TRY(F(&w->ts_sin, (size_t)TS_MAX * 320));
  JV_TRY(F(&w->ts_1, (size_t)TS_MAX * 1024));
  JV_TRY(F(&w->ts_mish, (size_t)TS_MAX * 1024));
  JV_TRY(F(&w->ts_emb, (size_t)TS_MAX * EST_NRES * 256));
  JV_TRY(F(&w->t_table, (size_t)w->max_steps));
  JV_TRY(F(&w->dt_table, (size_t)w->max_steps));
  JV_TRY(F(&w->cfg_table, (size_t)w->max_steps));
  JV_TRY(ws_alloc(c, R, reinterpret_cast<void**>(&w->rowmask)));
  JV_TRY(ws_alloc(c, R * sizeof(int), reinterpret_cast<void**>(&w->row_sample)));
  JV_TRY(ws_alloc(c, (size_t)B2 * sizeof(int), reinterpret_cast<void**>(&w->lens2)));
  JV_TRY(ws_alloc(c, (size_t)(B2 + 1) * sizeof(int), reinterpret_cast<void**>(&w->uoff)));
  JV_HIP(hipHostMalloc(reinterpret_cast<void**>(&w->h_lens), (size_t)B2 * sizeof(int), hipHostMallocDefault));
  JV_HIP(hipHostMalloc(reinterpret_cast<void**>(&w->h_uoff), (size_t)(B2 + 1) * sizeof(int), hipHostMallocDefault));
  JV_HIP(hipHostMalloc(reinterpret_cast<void**>(&w->h_sum), (size_t)B2 * sizeof(int), hipHostMallocDefault));
  JV_TRY(ws_alloc(c, (size_t)B2 * sizeof(int), reinterpret_cast<void**>(&w->t2m_lens)));
  JV_HIP(hipHostMalloc(reinterpret_cast<void**>(&w->h_y), (size_t)B2 * sizeof(int), hipHostMallocDefault));
  JV_TRY(ws_alloc(c, (size_t)c.max_batch * sizeof(PoolStepReq), reinterpret_cast<void**>(&w->pool_req)));
  JV_TRY(ws_alloc(c, sizeof(int), reinterpret_cast<void**>(&w->step_ctr)));
  JV_TRY(F(&w->t_cur, 1));
  JV_TRY(F(&w->dt_cur, 1));
  JV_TRY(F(&w->cfg_cur, 1));
  JV_HIP(hipStreamCreateWithFlags(&w->gstream, hipStreamNonBlocking));
  JV_HIP(hipEventCreateWithFlags(&w->ev_in, hipEventDisableTiming));
  JV_HIP(hipEventCreateWithFlags(&w->ev_out, hipEventDisableTiming));
  return JV_OK;
}

bool flow_has_graphs(const Context& c) { return c.flow && !c.flow->graphs.empty(); }

void flow_graphs_drop(Context& c) {
  if (!c.flow) return;
  for (auto& e : c.flow->graphs) {
    (void)hipGraphExecDestroy(e.exec);
    (void)hipGraphDestroy(e.graph);
  }
  c.flow->graphs.clear();
}

// new weights: rows of the attention buffer written under the old ones may exceed the new V bound (registry.hip)
void flow_ws_forget_attention(Context& c, hipStream_t st) {
  if (c.flow && c.flow->att) (void)hipMemsetAsync(c.flow->att, 0, (size_t)c.flow->rows_alloc * 512 * sizeof(float), st);
}

namespace {

// (t, dt, guidance rate) of the step the device-side counter points at, then advance it: the only step-dependent state of a solve
// (256 threads; emb_steps != null: the step's precomputed timestep embedding, [EST_NRES * 256] floats, moves to the fixed
// place the estimator's launches read it from -- their arguments are frozen inside a captured graph)
__global__ void step_advance_kernel(const float* __restrict__ t_table, const float* __restrict__ dt_table,
                                    const float* __restrict__ cfg_table, int* ctr, float* t_cur, float* dt_cur, float* cfg_cur,
                                    const float* __restrict__ emb_steps, float* __restrict__ emb_cur) {
  const int i = *ctr;
  if (emb_steps)
    for (int k = threadIdx.x; k < EST_NRES * 256; k += 256) emb_cur[k] = emb_steps[(long)i * EST_NRES * 256 + k];
  __syncthreads();      // every thread has read the counter
  if (threadIdx.x == 0) {
    *t_cur = t_table[i];
    *dt_cur = dt_table[i];
    *cfg_cur = cfg_table[i];
    *ctr = i + 1;
  }
}

// may a ragged batch of M rows take the compact geometry?  A read of the route such a call would take
bool flow_compact_ok(const Context& c, long M) { return est_route(c, M, false, true, c.attn_chunk).compact_ok; }

int check_shape(Context& c, int B2, int T) {
  if (!c.ready[MODEL_FLOW]) return fail(JV_ERR_STATE, "tts weights not finalized");
  if (B2 < 1 || T < 1) return fail(JV_ERR_ARG, "batch and frame count must be positive");
  if (B2 > 2 * c.max_batch || T > c.max_frames || flow_rows(B2, T) + 128 > c.flow->rows_alloc)
    return fail(JV_ERR_SHAPE, "batch/frames exceed the capacity given to jv_create");
  return JV_OK;
}

}  // namespace

// valid frames per row from the reference's float mask [B2,1,T] (1 = frame, 0 = padding; make_pad_mask gives prefixes)
__global__ void mask_to_lens_kernel(const float* __restrict__ mask, int T, int* __restrict__ lens) {
  const int b = blockIdx.x;
  int n = 0;
  for (int t = threadIdx.x; t < T; t += 64) n += mask[(long)b * T + t] != 0.f ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if (threadIdx.x == 0) lens[b] = n;
}

// tap (jv_flow_estimator_tap's ENTRY mode, else null): return behind the launches of that stage, its buffer in tap->out; `out` is
// then not written
int flow_estimator(Context& c, const float* x, const int* lens_dev, const float* mu, const float* t_dev, const float* spks,
                   const float* cond, int B2, int T, float* out, hipStream_t st, const float* mask_f32, const EstTap* tap) {
  JV_TRY(check_shape(c, B2, T));
  JV_TRY(est_tap_check(tap, B2, B2, T));
  FlowWs& w = *c.flow;
  Geo g{B2, T, T + FLOW_GAP, flow_rows(B2, T), w.rows_alloc, w.t_dev, 1};
  // channels-first [B2,80,T] inputs -> row buffers (reusing x/mu/cond, which hold 2B utterances here)
  JV_TRY(cf_to_rows(x, 80L * T, T, B2, 80, T, w.x, 80, 0, FLOW_G, g.S, 1.f, nullptr, st));
  JV_TRY(cf_to_rows(mu, 80L * T, T, B2, 80, T, w.mu, 80, 0, FLOW_G, g.S, 1.f, nullptr, st));
  JV_TRY(cf_to_rows(cond, 80L * T, T, B2, 80, T, w.cond, 80, 0, FLOW_G, g.S, 1.f, nullptr, st));
  if (mask_f32) hipLaunchKernelGGL(mask_to_lens_kernel, dim3(B2), dim3(64), 0, st, mask_f32, T, w.lens2);
  else if (lens_dev) JV_TRY(clamp_lens(lens_dev, B2, 1, T, w.lens2, st));
  else JV_TRY(fill_int(w.lens2, T, B2, st));
  JV_TRY(row_meta(w.rowmask, w.row_sample, w.lens2, B2, 1, FLOW_G, g.S, T, w.rows_alloc, 1, 0, st));
  JV_HIP(hipMemcpyAsync(w.t_dev, t_dev, sizeof(float) * B2, hipMemcpyDeviceToDevice, st));
  JV_TRY(assemble_xin_plain(w.x, w.mu, spks, w.cond, w.xin, B2, FLOW_G, g.S, T, g.M, st));
  if (tap && tap->id == JV_EST_TAP_XIN) return rows_to_cf(w.xin, 320, 0, FLOW_G, g.S, tap->out, 320L * T, B2, 320, T, w.lens2, st);
  JV_HIP(hipMemsetAsync(w.amax, 0, sizeof(float) * 3 * w.amax_stride, st));
  JV_TRY(estimator_body(c, g, est_route(c, g.M, false, false, c.attn_chunk), st, tap));
  if (tap) return JV_OK;
  return rows_to_cf(w.d, 80, 0, FLOW_G, g.S, out, 80L * T, B2, 80, T, nullptr, st);
}

namespace {

// ---- the three parts of a solve that cfm_solve and cfm_solve_prompted share: schedule, geometry, Euler loop ----------------
// The entries differ in what they pack into the row buffers before the loop and in what they unpack after it.

// The guidance mode of the context (jv_flow_set_guidance) against a solve of n_timesteps steps: a schedule has one rate per step.
// Called by every entry before its first launch.
int guidance_check(const Context& c, const char* who, int n_timesteps) {
  if (c.guidance.size() > 1 && (int)c.guidance.size() != n_timesteps) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: n_timesteps = %d, but the guidance schedule (jv_flow_set_guidance) holds %d rates: one per Euler step",
             who, n_timesteps, (int)c.guidance.size());
    return fail(JV_ERR_ARG, msg);
  }
  return JV_OK;
}

// The solver mode of the context (jv_flow_set_solver) against a solve of n_timesteps steps: the tables hold one slot per estimator
// evaluation, two per step of a second-order solver.  Called by every entry before its first launch, after its own range check.
int solver_check(const Context& c, const char* who, int n_timesteps) {
  if (c.solver != JV_SOLVER_EULER && 2L * n_timesteps > c.flow->max_steps) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: n_timesteps = %d with the %s solver (jv_flow_set_solver) is %ld estimator evaluations, the limit is %d",
             who, n_timesteps, c.solver == JV_SOLVER_MIDPOINT ? "midpoint" : "Heun", 2L * n_timesteps, c.flow->max_steps);
    return fail(JV_ERR_ARG, msg);
  }
  return JV_OK;
}

// the rate of step k: 0.7 where no mode is set (flow_matching.py:252-258, inference_cfg_rate of configs/base.yaml)
float guidance_rate(const Context& c, int k) {
  return c.guidance.empty() ? 0.7f : c.guidance.size() == 1 ? c.guidance[0] : c.guidance[(size_t)k];
}

// Does the solve lay out unconditional twins at all?  Not where every step's rate is exactly 0 (JV_NO_TWIN_DROP=1: always)
bool solve_twins(const Context& c, int n_timesteps) {
  if (c.no_twin_drop) return true;
  for (int k = 0; k < n_timesteps; ++k)
    if (guidance_rate(c, k) != 0.f) return true;
  return false;
}

// (t, dt, guidance rate) of every step -> w.t_table / w.dt_table / w.cfg_table.  tt / dts are the caller's: pageable staging
// that must live until the solve's one synchronisation has consumed the copies (the rates ride behind dts in the same vector).
int solve_schedule(const Context& c, FlowWs& w, int n_timesteps, const float* t_span_host, std::vector<float>& tt,
                   std::vector<float>& dts, hipStream_t st) {
  std::vector<float> ts(n_timesteps + 1);
  tt.resize(n_timesteps);
  dts.resize(2 * (size_t)n_timesteps);
  for (int k = 0; k < n_timesteps; ++k) dts[(size_t)n_timesteps + k] = guidance_rate(c, k);
  // cosine schedule and the reference's running (t, dt) recurrence, in fp32 (flow_matching.py:230,260-263,387-389)
  if (t_span_host) {
    for (int i = 0; i <= n_timesteps; ++i) ts[i] = t_span_host[i];
  } else {
    const int steps = n_timesteps + 1;
    const float step = 1.0f / (float)(steps - 1);
    for (int i = 0; i < steps; ++i) {
      const float lin = i < steps / 2 ? step * (float)i : 1.0f - step * (float)(steps - 1 - i);
      ts[i] = 1.0f - cosf(lin * 0.5f * 3.14159265358979323846f);
    }
  }
  {
    float t = ts[0], dt = ts[1] - ts[0];
    for (int s = 1; s <= n_timesteps; ++s) {
      tt[s - 1] = t;
      dts[s - 1] = dt;
      t = t + dt;
      if (s < n_timesteps) dt = ts[s + 1] - t;
    }
  }
  // A second-order solver (jv_flow_set_solver): one table slot per EVALUATION, step k at slots 2k and 2k + 1 -- the second time
  // is t + 0.5f dt (midpoint) or t + dt, the next step's t under the recurrence above (Heun); the coefficient of a stage's update
  // is 0.5f dt in the half stage (midpoint's first, Heun's second), dt in the other; the step's rate holds for both evaluations
  int n_evals = n_timesteps;
  if (c.solver != JV_SOLVER_EULER) {
    const bool mid = c.solver == JV_SOLVER_MIDPOINT;
    n_evals = 2 * n_timesteps;
    std::vector<float> t2((size_t)n_evals), c2(2 * (size_t)n_evals);
    for (int k = 0; k < n_timesteps; ++k) {
      const float t = tt[k], dt = dts[k], half = 0.5f * dt, rate = dts[(size_t)n_timesteps + k];
      t2[2 * k] = t;
      t2[2 * k + 1] = mid ? t + half : t + dt;
      c2[2 * k] = mid ? half : dt;
      c2[2 * k + 1] = mid ? dt : half;
      c2[(size_t)n_evals + 2 * k] = c2[(size_t)n_evals + 2 * k + 1] = rate;
    }
    tt.swap(t2);
    dts.swap(c2);
  }
  JV_HIP(hipMemcpyAsync(w.t_table, tt.data(), sizeof(float) * n_evals, hipMemcpyHostToDevice, st));
  JV_HIP(hipMemcpyAsync(w.dt_table, dts.data(), sizeof(float) * n_evals, hipMemcpyHostToDevice, st));
  JV_HIP(hipMemcpyAsync(w.cfg_table, dts.data() + n_evals, sizeof(float) * n_evals, hipMemcpyHostToDevice, st));
  return JV_OK;
}

// COMPACT geometry: every utterance (and its CFG twin) gets its own frames + the gap, nothing is padded to the longest;
// taken when it saves at least 8 % of the rows and the shorter batch still fills the row-owning kernels.  All per-row
// arithmetic is the uniform geometry's (a row's sums do not depend on where the row sits): the same bits per utterance.
// h_lens: the B sequence lengths on the host (after the solve's synchronisation).
// the rule alone, on host arrays (cfm_pool_step lays a step out by it as well): uoff[B2 + 1] receives the first rows; true = compact
// B2: the samples laid out, 2B, or B for a solve without guidance (M_uniform is then that geometry's row count as well)
bool compact_plan(const Context& c, long M_uniform, const int* h_lens, int B, int B2, int T, int* uoff, long* rows, long* frames_out) {
  long r = FLOW_G, frames = 0;
  for (int b2 = 0; b2 < B2; ++b2) {
    const int len = std::min(std::max(h_lens[b2 % B], 0), T);
    uoff[b2] = (int)r;
    r += len + FLOW_GAP;
    frames += len;
  }
  uoff[B2] = (int)r;
  *rows = r; *frames_out = frames;
  return r * 100 <= M_uniform * 92 && flow_compact_ok(c, r);
}

int solve_compact(Context& c, Geo& g, const int* h_lens, int B, int T, hipStream_t st) {
  FlowWs& w = *c.flow;
  long r = 0, frames = 0;
  if (compact_plan(c, g.M, h_lens, B, g.B2, T, w.h_uoff, &r, &frames)) {
    JV_HIP(hipMemcpyAsync(w.uoff, w.h_uoff, sizeof(int) * (g.B2 + 1), hipMemcpyHostToDevice, st));      // (pinned: stays valid)
    g.M = r; g.uoff = w.uoff; g.alg_rows = frames;
  }
  return JV_OK;
}

// After a solve's shared first step (solve_loop): the B - 1 twin slots the step did not compute take slot B's running maxima,
// which is what B identical twins would have left in them -- the later steps derive their fp16x3 scales from these slots
__global__ void amax_share_kernel(float* __restrict__ amax, int stride, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // [3 buffers][B - 1 slots]
  if (i >= 3 * (B - 1)) return;
  const int k = i / (B - 1), j = i - k * (B - 1);
  amax[k * stride + B + 1 + j] = amax[k * stride + B];
}

// are the B clamped lengths the host holds all the same?  (null: no lengths were passed, every utterance has T frames)
bool lens_all_equal(const int* h_lens, int B, int T) {
  if (!h_lens) return true;
  const int l0 = std::min(std::max(h_lens[0], 0), T);
  for (int b = 1; b < B; ++b)
    if (std::min(std::max(h_lens[b], 0), T) != l0) return false;
  return true;
}

// What cfm_solve does between its schedule and its noise, shared with jv_flow_estimator_tap's STEP mode: the geometry of a batch of
// B utterances laid out as g.B2 samples (compact where compact_plan says so), the clamped lengths, the row tables, and mu / cond as
// rows.  Synchronises `st` once (the lengths of a ragged candidate come down with it; a caller's pageable staging is consumed by
// it).  *clens: the lengths a further cf_to_rows of the call takes (compact: only an utterance's own frames are written);
// *lens_equal: the host knows the B lengths to be the same
int solve_pack(Context& c, Geo& g, const float* mu, const int* lens_dev, const float* cond, int B, int T, const int** clens,
               bool* lens_equal, hipStream_t st) {
  FlowWs& w = *c.flow;
  // Ragged batch?  The lengths come down with the synchronisation below (which the staging vectors need anyway): B ints.
  const bool ragged_candidate = lens_dev && B > 1 && flow_compact_ok(c, g.M);
  if (ragged_candidate) JV_HIP(hipMemcpyAsync(w.h_lens, lens_dev, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  // pageable-host staging vectors die at scope exit: make sure the copies have been consumed
  JV_HIP(hipStreamSynchronize(st));
  if (ragged_candidate) JV_TRY(solve_compact(c, g, w.h_lens, B, T, st));

  // pack: lengths (duplicated for the CFG twin rows), masks, row-layout mu / cond
  if (lens_dev) {
    JV_TRY(clamp_lens(lens_dev, B, g.B2 / B, T, w.lens2, st));      // (the layout above used the same clamp on the host copy)
  } else {
    JV_TRY(fill_int(w.lens2, T, g.B2, st));
  }
  *clens = g.uoff ? w.lens2 : nullptr;
  JV_TRY(row_meta(w.rowmask, w.row_sample, w.lens2, g.B2, 1, FLOW_G, g.S, T, w.rows_alloc, 1, 0, st, g.uoff));
  JV_TRY(cf_to_rows(mu, 80L * T, T, B, 80, T, w.mu, 80, 0, FLOW_G, g.S, 1.f, *clens, st, g.uoff));
  JV_TRY(cf_to_rows(cond, 80L * T, T, B, 80, T, w.cond, 80, 0, FLOW_G, g.S, 1.f, *clens, st, g.uoff));
  // (equal lengths: known where none were passed or where the ragged check brought them down)
  *lens_equal = !lens_dev || (ragged_candidate && lens_all_equal(w.h_lens, B, T));
  return JV_OK;
}

// the Euler loop on packed row buffers (w.mu, w.cond, w.x = z, w.lens2, row metadata): the result is left in w.x
// lens_equal: the host knows that all B utterances have the same number of frames (it learns so without a copy of its own)
// g.B2 = 2B: the rows hold every utterance's unconditional twin; g.B2 = B (solve_twins: every rate is 0): none was laid out
int solve_loop(Context& c, Geo& g, const float* spks, int B, int T, int n_timesteps, bool lens_equal, hipStream_t st) {
  FlowWs& w = *c.flow;
  const bool twins = g.B2 == 2 * B;
  JV_HIP(hipMemsetAsync(w.step_ctr, 0, sizeof(int), st));
  JV_HIP(hipMemsetAsync(w.amax, 0, sizeof(float) * 3 * w.amax_stride, st));      // trunk bounds: maxima over the whole solve
  JV_HIP(hipMemcpyAsync(w.spks, spks, sizeof(float) * 80 * B, hipMemcpyDeviceToDevice, st));
  g.t_ptr = w.t_cur;   // the same t for all 2B rows (stride 0)
  // Every step's t is on the device already and is the same for all rows: the n embeddings are three GEMMs of n rows HERE
  // instead of three GEMMs of 2B identical rows inside every step -- K = 1024 contractions of one row tile, 20 - 48 us each
  // at any batch size, 1.2 ms of serial launches per solve (JV_NO_TEMB_PRE=1: per step, as jv_flow_estimator_masked does)
  // A second-order solver (jv_flow_set_solver) evaluates the estimator twice per step: solve_schedule laid the tables out per
  // evaluation, so the embeddings ahead of the loop cover all 2n times where 2n <= TS_MAX
  const int n_evals = c.solver == JV_SOLVER_EULER ? n_timesteps : 2 * n_timesteps;
  g.temb_pre = !c.no_temb_pre && n_evals <= TS_MAX;
  if (g.temb_pre) JV_TRY(time_embedding(c, w.t_table, 1, n_evals, w.ts_sin, w.ts_1, w.ts_mish, w.ts_emb, st));
  const EstRoute route = est_route(c, g.M, g.temb_pre, g.uoff != nullptr, c.attn_chunk);      // one route for every step (and for a captured one)
  // one Euler step over `gg` / `rt` with `ntwin` unconditional twins: B of them, the one shared twin of step 0 (after which the
  // slots it stands for take its maxima), or none in a step whose guidance rate is 0 (the row tables were built for 2B samples:
  // the first B + 1, or B, are a prefix of them).  The step's rate comes through w.cfg_cur as its dt comes through w.dt_cur
  auto euler_step = [&](hipStream_t s, const Geo& gg, const EstRoute& rt, int ntwin) -> int {
    const bool one_twin = ntwin == 1 && B > 1;
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(256), 0, s, w.t_table, w.dt_table, w.cfg_table, w.step_ctr, w.t_cur,
                       w.dt_cur, w.cfg_cur, g.temb_pre ? w.ts_emb : nullptr, w.temb);
    JV_TRY(assemble_xin(w.x, w.mu, w.spks, w.cond, w.xin, B, ntwin, FLOW_G, gg.S, T, gg.M, s, gg.uoff, w.row_sample, w.rowmask));
    JV_TRY(estimator_body(c, gg, rt, s));
    JV_TRY(euler_cfg(w.x, w.d, B, FLOW_G, gg.S, T, w.dt_cur, 0, w.cfg_cur, s, gg.uoff, w.lens2, one_twin, ntwin == 0));
    if (one_twin) {
      hipLaunchKernelGGL(amax_share_kernel, dim3((unsigned)cdiv(3 * (B - 1), 64)), dim3(64), 0, s, w.amax, w.amax_stride, B);
      JV_HIP(hipGetLastError());
    }
    return JV_OK;
  };
  auto same_resnets = [](const EstRoute& a, const EstRoute& b) {
    for (int i = 0; i < EST_NRES; ++i)
      if (a.stage[i].res != b.stage[i].res || a.stage[i].rows != b.stage[i].rows) return false;
    return true;
  };
  // NO twin in a step whose guidance rate is exactly 0: (1 + 0) d_c - 0 d_u needs no d_u, so the step runs on the B conditional
  // samples -- the prefix of the 2B-sample rows, as the shared first step below runs on a prefix of B + 1 -- and x += dt d.
  // A solve whose rates are ALL 0 arrives here with g laid out for B samples and takes every step that way on `route`.  A solve
  // with mixed rates changes geometry between steps and is bound by the rule the shared first step states: both geometries on the
  // row-owning side of the split-K seam, the same resnet launches in both (trunk buffers, running maxima), uniform rows.  Where
  // the rule is not met the step keeps its twins and euler_cfg with rate 0 gives the same x: the only degradation.
  // JV_NO_TWIN_DROP=1: twins in every step.  (DESIGN.md 5 "Guidance")
  std::vector<char> drop((size_t)n_timesteps, twins ? 0 : 1);
  Geo gB = g;
  EstRoute routeB = route;
  if (twins && !c.no_twin_drop) {
    bool any = false;
    for (int k = 0; k < n_timesteps; ++k) any = any || guidance_rate(c, k) == 0.f;
    const long MB = flow_rows(B, T);
    if (any && !g.uoff && MB > PARTIAL_ROWS && rowgemm_tile((int)MB) != 0) {
      gB.B2 = B; gB.M = MB; gB.alg_rows = 0;      // (the profiler's frames: B T)
      routeB = est_route(c, MB, g.temb_pre, false, c.attn_chunk);      // once per geometry, not per step
      if (!same_resnets(routeB, route)) routeB = est_route(c, MB, g.temb_pre, false, c.attn_chunk, false);
      if (same_resnets(routeB, route))
        for (int k = 0; k < n_timesteps; ++k) drop[(size_t)k] = guidance_rate(c, k) == 0.f;
    }
  }
  bool any_drop = false;
  for (int k = 0; k < n_timesteps; ++k) any_drop = any_drop || drop[(size_t)k];
  // step k in the form its rate allows (eager)
  auto step_k = [&](int k) -> int { return drop[(size_t)k] ? euler_step(st, twins ? gB : g, twins ? routeB : route, 0) : euler_step(st, g, route, B); };
  // MIDPOINT / HEUN (jv_flow_set_solver; DESIGN.md 5 "Solver"): two evaluations per step, each the Euler step's launches with
  // solver_stage in euler_cfg's place -- the first saves x (and, Heun, its slope) and leaves the stage point in w.x, the second
  // forms the new x from the saved state.  step_advance_kernel advances per evaluation; the step's rate, and so its geometry
  // (drop[k], by the rule above), holds for both.  Always eager, on 2B (or B) samples: step 0's first evaluation alone has
  // identical twins, and the captured graph is a 2B EULER step -- it keeps replaying for Euler solves only.  The running maxima
  // accumulate over all evaluations.
  if (c.solver != JV_SOLVER_EULER) {
    const bool mid = c.solver == JV_SOLVER_MIDPOINT;
    for (int k = 0; k < n_timesteps; ++k) {
      const bool no_twin = drop[(size_t)k];
      const Geo& gg = no_twin && twins ? gB : g;
      const EstRoute& rt = no_twin && twins ? routeB : route;
      for (int e = 0; e < 2; ++e) {
        hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(256), 0, st, w.t_table, w.dt_table, w.cfg_table, w.step_ctr, w.t_cur,
                           w.dt_cur, w.cfg_cur, g.temb_pre ? w.ts_emb : nullptr, w.temb);
        JV_TRY(assemble_xin(w.x, w.mu, w.spks, w.cond, w.xin, B, no_twin ? 0 : B, FLOW_G, gg.S, T, gg.M, st, gg.uoff, w.row_sample, w.rowmask));
        JV_TRY(estimator_body(c, gg, rt, st));
        const int stage = mid ? (e == 0 ? STAGE_MID1 : STAGE_MID2) : (e == 0 ? STAGE_HEUN1 : STAGE_HEUN2);
        JV_TRY(solver_stage(w.x, w.x0, w.k1, w.d, B, FLOW_G, gg.S, T, w.dt_cur, w.cfg_cur, stage, no_twin ? SOLVER_TWIN_NONE : SOLVER_TWIN_EACH,
                            st, gg.uoff, w.lens2));
      }
    }
#ifdef JV_TUNING
    JV_TRY(est_stamps_dump(c, g, st));
#endif
    return JV_OK;
  }
  int done = 0;      // steps enqueued so far
  // ONE unconditional twin for the first step.  Every utterance starts from the same noise prefix, a twin has mu = spks = cond = 0
  // and t is one scalar: with equal lengths the B twins of step 0 are one sample B times over, so the step runs on B + 1 samples
  // -- the twin at slot B, reading x of utterance 0 -- and every utterance's CFG update reads that slot.  An utterance's bits do
  // not depend on the batch or the tile height, but they do differ across the split-K seam: the shorter geometry has to stay on
  // the row-owning side of it as well.  JV_NO_CFG_SHARE=1: 2B samples in every step.  
  const long M0 = flow_rows(B + 1, T);
  if (twins && !drop[0] && !c.no_cfg_share && lens_equal && B >= 2 && !g.uoff && M0 > PARTIAL_ROWS && rowgemm_tile((int)M0) != 0) {
    Geo g0 = g;
    g0.B2 = B + 1; g0.M = M0; g0.alg_rows = 0;      // (the profiler's frames: (B + 1) T)
    // ... and every resnet has to take the same launches in both geometries: the one-launch form (which has to fit its rounds,
    // rowres_fits: a function of the row count) alternates the trunk between w.h and w.h2, the others keep it in w.h, and the
    // running maxima are kept per BUFFER -- a step 0 on other buffers would leave other maxima, the conditional samples'
    // included, to the later steps.  Where only the shorter geometry would fit the one-launch form, step 0 does without it
    EstRoute route0 = est_route(c, M0, g.temb_pre, false, c.attn_chunk);
    if (!same_resnets(route0, route)) route0 = est_route(c, M0, g.temb_pre, false, c.attn_chunk, false);
    if (same_resnets(route0, route)) {      // (always eager: a captured step is a 2B step)
      JV_TRY(euler_step(st, g0, route0, 1));
      done = 1;
    }
  }
  // The in-library profiler brackets every launch with events, which a capture would turn into graph nodes: eager then.
  // ... and a captured step is a 2B step: a solve with a step without twins is eager throughout, so no 2B graph ever replays for it
  const bool use_graph = c.step_graphs && !prof_on() && n_timesteps > 1 && !g.uoff && !any_drop;      // (a captured step is keyed by (B, T): uniform geometry only)
  if (!use_graph) {
    for (int s = done; s < n_timesteps; ++s) JV_TRY(step_k(s));
  } else {
    FlowWs::StepGraph* sg = nullptr;
    for (auto& e : w.graphs)
      if (e.B == B && e.T == T && e.chunk == c.attn_chunk && e.pre == (int)g.temb_pre) sg = &e;
    // first solve of this geometry: one 2B step runs eagerly (it also performs the one-time kernel attribute setup), the next
    // one is captured; it does not execute during capture, so the replay loop starts from it
    if (!sg) {
      JV_TRY(euler_step(st, g, route, B));
      ++done;
    }
    JV_HIP(hipEventRecord(w.ev_in, st));
    JV_HIP(hipStreamWaitEvent(w.gstream, w.ev_in, 0));
    if (!sg) {
      JV_HIP(hipStreamBeginCapture(w.gstream, hipStreamCaptureModeThreadLocal));
      const int rc = euler_step(w.gstream, g, route, B);
      hipGraph_t graph = nullptr;
      const hipError_t ce = hipStreamEndCapture(w.gstream, &graph);
      if (rc != JV_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (ce != hipSuccess || !graph) return fail(JV_ERR_HIP, "cfm_solve: stream capture of the Euler step failed");
      hipGraphExec_t exec = nullptr;
      if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(graph);
        return fail(JV_ERR_HIP, "cfm_solve: hipGraphInstantiate failed");
      }
      if (w.graphs.size() >= 16) {   // bounded cache: drop the oldest geometry
        (void)hipGraphExecDestroy(w.graphs.front().exec);
        (void)hipGraphDestroy(w.graphs.front().graph);
        w.graphs.erase(w.graphs.begin());
      }
      w.graphs.push_back({B, T, c.attn_chunk, (int)g.temb_pre, graph, exec});
      sg = &w.graphs.back();
    }
    for (int s = done; s < n_timesteps; ++s) JV_HIP(hipGraphLaunch(sg->exec, w.gstream));
    JV_HIP(hipEventRecord(w.ev_out, w.gstream));
    JV_HIP(hipStreamWaitEvent(st, w.ev_out, 0));
  }
#ifdef JV_TUNING
  JV_TRY(est_stamps_dump(c, g, st));
#endif
  return JV_OK;
}

}  // namespace

int cfm_solve(Context& c, const float* mu, const int* lens_dev, const float* spks, const float* cond, int B, int T,
              int n_timesteps, float temperature, const float* t_span_host, float* mel, hipStream_t st) {
  JV_TRY(check_shape(c, 2 * B, T));
  if (!c.noise_loaded) return fail(JV_ERR_STATE, "CFM noise tensor not loaded (jv_load_noise)");
  if (T > NOISE_FRAMES) return fail(JV_ERR_SHAPE, "more frames than the fixed noise tensor holds (15000)");
  FlowWs& w = *c.flow;
  if (n_timesteps < 1 || n_timesteps > w.max_steps) return fail(JV_ERR_ARG, "n_timesteps out of range");
  JV_TRY(guidance_check(c, "jv_cfm_solve", n_timesteps));
  JV_TRY(solver_check(c, "jv_cfm_solve", n_timesteps));
  const int B2 = solve_twins(c, n_timesteps) ? 2 * B : B;      // samples laid out: no twin where no step has guidance
  Geo g{B2, T, T + FLOW_GAP, flow_rows(B2, T), w.rows_alloc, nullptr, 0};

  std::vector<float> tt, dts;
  JV_TRY(solve_schedule(c, w, n_timesteps, t_span_host, tt, dts, st));
  bool lens_equal = false;
  const int* clens = nullptr;
  JV_TRY(solve_pack(c, g, mu, lens_dev, cond, B, T, &clens, &lens_equal, st));      // (its synchronisation has consumed tt / dts)
  // z = rand_noise[:, :, :T] * temperature, the same prefix for every utterance (flow_matching.py:385)
  JV_TRY(cf_to_rows(c.noise, 0, NOISE_FRAMES, B, 80, T, w.x, 80, 0, FLOW_G, g.S, temperature, clens, st, g.uoff));

  JV_TRY(solve_loop(c, g, spks, B, T, n_timesteps, lens_equal, st));
  // unpack
  return rows_to_cf(w.x, 80, 0, FLOW_G, g.S, mel, 80L * T, B, 80, T, lens_dev ? w.lens2 : nullptr, st, g.uoff);
}

// jv_flow_estimator_tap.  ENTRY: flow_estimator with the tap.  STEP: ONE evaluation as solve_loop's euler_step runs it inside
// cfm_solve -- cfm_solve's checks and pack (solve_pack: the compact geometry exactly where a solve takes it), x as given in the
// noise's place, B unconditional twins, one t whose embedding is made ahead of the evaluation (time_embedding over n = 1 straight
// into w.temb, where step_advance_kernel would move the step's row), the maxima zeroed as at the head of a solve, the route of a
// solve's steps -- up to the tap.  No CFG update: the tap is the evaluation's own
int flow_estimator_tap(Context& c, int mode, const float* x, const int* lens_dev, const float* mu, const float* t_dev,
                       const float* spks, const float* cond, int B, int T, int tap_id, float* out, long out_floats, hipStream_t st) {
  const EstTap tap{tap_id, out, out_floats};
  if (mode == JV_EST_MODE_ENTRY) return flow_estimator(c, x, lens_dev, mu, t_dev, spks, cond, B, T, nullptr, st, nullptr, &tap);
  if (mode != JV_EST_MODE_STEP) return fail(JV_ERR_ARG, "jv_flow_estimator_tap: mode is JV_EST_MODE_ENTRY or JV_EST_MODE_STEP");
  JV_TRY(check_shape(c, 2 * B, T));
  JV_TRY(est_tap_check(&tap, 2 * B, 1, T));
  FlowWs& w = *c.flow;
  Geo g{2 * B, T, T + FLOW_GAP, flow_rows(2 * B, T), w.rows_alloc, nullptr, 0};
  bool lens_equal = false;
  const int* clens = nullptr;
  JV_TRY(solve_pack(c, g, mu, lens_dev, cond, B, T, &clens, &lens_equal, st));
  JV_TRY(cf_to_rows(x, 80L * T, T, B, 80, T, w.x, 80, 0, FLOW_G, g.S, 1.f, clens, st, g.uoff));
  JV_HIP(hipMemsetAsync(w.amax, 0, sizeof(float) * 3 * w.amax_stride, st));
  JV_HIP(hipMemcpyAsync(w.spks, spks, sizeof(float) * 80 * B, hipMemcpyDeviceToDevice, st));
  g.t_ptr = w.t_cur;
  g.temb_pre = true;
  JV_TRY(time_embedding(c, t_dev, 1, 1, w.tsin, w.t1, w.tmish, w.temb, st, est_tap_time_stages(&tap)));
  const EstRoute route = est_route(c, g.M, true, g.uoff != nullptr, c.attn_chunk);
  JV_TRY(assemble_xin(w.x, w.mu, w.spks, w.cond, w.xin, B, B, FLOW_G, g.S, T, g.M, st, g.uoff, w.row_sample, w.rowmask));
  if (tap.id == JV_EST_TAP_XIN) return rows_to_cf(w.xin, 320, 0, FLOW_G, g.S, tap.out, 320L * T, 2 * B, 320, T, w.lens2, st, g.uoff);
  return estimator_body(c, g, route, st, &tap);
}

// The voice-cloning batch: utterance b's sequence is [prompt_b | text_b], p_b + y_b frames, with its own split point
// (jyutvoice_tts.py:213-244 looped over the utterances).  The same schedule, geometry rule and Euler loop as cfm_solve on the
// summed lengths; only the pack (prompt rows copied frame-major, text rows transposed from mu_y, cond zero behind the prompt)
// and the unpack (frames p_b .. p_b + y_b - 1, left-aligned) are its own.
int cfm_solve_prompted(Context& c, const float* mu_y, const int* y_lens, const float* prompt_h, const float* prompt_feat,
                       const int* prompt_lens, const float* spks, int B, int Ty, int Ph, int Pf, int n_timesteps,
                       float temperature, const float* t_span_host, float* mel, hipStream_t st) {
  if (!c.ready[MODEL_FLOW]) return fail(JV_ERR_STATE, "tts weights not finalized");
  if (B < 1 || Ty < 1 || Ph < 0 || Pf < 0) return fail(JV_ERR_ARG, "jv_cfm_solve_prompted: B, Ty must be positive, Ph, Pf non-negative");
  if (B > c.max_batch) return fail(JV_ERR_SHAPE, "batch/frames exceed the capacity given to jv_create");
  if (!c.noise_loaded) return fail(JV_ERR_STATE, "CFM noise tensor not loaded (jv_load_noise)");
  FlowWs& w = *c.flow;
  if (n_timesteps < 1 || n_timesteps > w.max_steps) return fail(JV_ERR_ARG, "n_timesteps out of range");
  if ((reinterpret_cast<uintptr_t>(prompt_h) | reinterpret_cast<uintptr_t>(prompt_feat)) & 15)
    return fail(JV_ERR_ARG, "jv_cfm_solve_prompted: prompt_h / prompt_feat must be 16-byte aligned");
  JV_TRY(guidance_check(c, "jv_cfm_solve_prompted", n_timesteps));
  JV_TRY(solver_check(c, "jv_cfm_solve_prompted", n_timesteps));
  const int B2 = solve_twins(c, n_timesteps) ? 2 * B : B, Pmax = std::min(Ph, Pf);

  std::vector<float> tt, dts;
  JV_TRY(solve_schedule(c, w, n_timesteps, t_span_host, tt, dts, st));
  // both length vectors always come down (2B ints): they are validated here, before anything is launched on them
  JV_HIP(hipMemcpyAsync(w.h_lens, y_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipMemcpyAsync(w.h_lens + B, prompt_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipStreamSynchronize(st));
  // A wrong length here is a wrong split point between prompt and text, which a clamp would turn into other frames silently:
  // rejected on the host (the entries without a prompt clamp instead, jyutvoice_hip.h "Lengths").
  int T = 0;
  for (int b = 0; b < B; ++b) {
    const int y = w.h_lens[b], p = w.h_lens[B + b];
    char msg[160];
    if (p < 0 || p > Pmax) {
      snprintf(msg, sizeof msg, "jv_cfm_solve_prompted: utterance %d: prompt length %d outside [0, min(Ph, Pf) = %d]", b, p, Pmax);
      return fail(JV_ERR_ARG, msg);
    }
    if (y < 0 || y > Ty) {
      snprintf(msg, sizeof msg, "jv_cfm_solve_prompted: utterance %d: %d frames outside [0, Ty = %d]", b, y, Ty);
      return fail(JV_ERR_ARG, msg);
    }
    w.h_sum[b] = w.h_sum[B + b] = p + y;
    T = std::max(T, p + y);
  }
  JV_TRY(check_shape(c, 2 * B, T));      // (the capacity counts twins whether or not this solve lays them out)
  if (T > NOISE_FRAMES) return fail(JV_ERR_SHAPE, "more frames than the fixed noise tensor holds (15000)");
  Geo g{B2, T, T + FLOW_GAP, flow_rows(B2, T), w.rows_alloc, nullptr, 0};
  if (B > 1 && flow_compact_ok(c, g.M)) JV_TRY(solve_compact(c, g, w.h_sum, B, T, st));

  // pack
  JV_HIP(hipMemcpyAsync(w.lens2, w.h_sum, sizeof(int) * B2, hipMemcpyHostToDevice, st));      // (pinned: stays valid)
  const int* const clens = g.uoff ? w.lens2 : nullptr;
  JV_TRY(row_meta(w.rowmask, w.row_sample, w.lens2, B2, 1, FLOW_G, g.S, T, w.rows_alloc, 1, 0, st, g.uoff));
  JV_TRY(pack_prompted(mu_y, Ty, prompt_h, Ph, prompt_feat, Pf, prompt_lens, w.lens2, B, T, w.mu, w.cond, FLOW_G, g.S, st, g.uoff));
  // z = rand_noise[:, :, :p_b + y_b] * temperature: column j is frame j of the utterance's own sequence (flow_matching.py:385)
  JV_TRY(cf_to_rows(c.noise, 0, NOISE_FRAMES, B, 80, T, w.x, 80, 0, FLOW_G, g.S, temperature, clens, st, g.uoff));

  JV_TRY(solve_loop(c, g, spks, B, T, n_timesteps, lens_all_equal(w.h_sum, B, T), st));
  // unpack: the generated frames only (jyutvoice_tts.py:244 `decoder_outputs[:, :, mel_len1:]`), zeros behind y_b
  return rows_to_cf_from(w.x, 80, FLOW_G, g.S, prompt_lens, y_lens, mel, 80L * Ty, B, 80, Ty, st, g.uoff);
}

// ---- in-flight batching (jv_cfm_pool_admit / _step / _fetch; kernels: cfmpool.hip) ---------------------------------------------
// Between two Euler steps a solve's state is x, the running trunk maxima and a step counter, and the estimator takes one t per
// sample: the utterances of one evaluation need not be at the same step.  A request's state lives in the caller's pools; a step
// gathers the listed slots into the workspace rows, runs assemble_xin and estimator_body as solve_loop's step does -- with t per
// sample, so without the precomputed embedding and therefore without the whole-resnet launch (est_route: RES_ONE needs temb_pre)
// -- and applies the update with the request's own dt while scattering x back.  The maxima travel with the request: its scales
// depend on that request alone, whoever held its slot or its workspace position before.
// Every call checks all of its arguments before its first launch, never synchronises, and reads its host arrays only until it
// returns (their values travel as kernel arguments).
// jv_cfm_pool_step_s: a request on a second-order solver takes two pool steps per solver step, and a pool step takes every request
// at the stage of its OWN solver (PoolStepReq::stage and its coefficient).  pool_x always holds the estimator's next input -- the
// stage point xs between a step's two stages -- so the gather is the same for every stage; only the scatter differs
// (pool_stage_scatter: x0 and k1 of a request wait in the caller's pool_x0 / pool_k1).

namespace {

int pool_check_pools(const char* who, const void* a, const void* b, const void* c3, const void* d, const void* e, int slots, int Tcap) {
  char msg[160];
  if (slots < 1 || Tcap < 1) {
    snprintf(msg, sizeof msg, "%s: slots and Tcap must be positive", who);
    return fail(JV_ERR_ARG, msg);
  }
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c3) | reinterpret_cast<uintptr_t>(d) |
       reinterpret_cast<uintptr_t>(e)) & 15) {
    snprintf(msg, sizeof msg, "%s: the pools must be 16-byte aligned", who);
    return fail(JV_ERR_ARG, msg);
  }
  return JV_OK;
}

// slot in range and named once among the call's requests (seen: [slots], zeroed by the caller)
int pool_check_slot(const char* who, int b, int slot, int slots, std::vector<char>& seen) {
  char msg[160];
  if (slot < 0 || slot >= slots) {
    snprintf(msg, sizeof msg, "%s: request %d: slot %d outside [0, %d)", who, b, slot, slots);
    return fail(JV_ERR_ARG, msg);
  }
  if (seen[slot]) {
    snprintf(msg, sizeof msg, "%s: request %d: slot %d is named twice", who, b, slot);
    return fail(JV_ERR_ARG, msg);
  }
  seen[slot] = 1;
  return JV_OK;
}

}  // namespace

int cfm_pool_admit(Context& c, const float* mu_y, const float* prompt_h, const float* prompt_feat, const float* spks,
                   const int* h_ylens, const int* h_plens, const int* h_slots, const float* h_temps, int B, int Ty, int Ph, int Pf,
                   float* pool_x, float* pool_mu, float* pool_cond, float* pool_spks, float* pool_amax, int slots, int Tcap,
                   hipStream_t st) {
  const char* who = "jv_cfm_pool_admit";
  if (!c.ready[MODEL_FLOW]) return fail(JV_ERR_STATE, "tts weights not finalized");
  if (!c.noise_loaded) return fail(JV_ERR_STATE, "CFM noise tensor not loaded (jv_load_noise)");
  if (B < 1 || Ty < 0 || Ph < 0 || Pf < 0) return fail(JV_ERR_ARG, "jv_cfm_pool_admit: B must be positive, Ty, Ph, Pf non-negative");
  JV_TRY(pool_check_pools(who, pool_x, pool_mu, pool_cond, pool_spks, spks, slots, Tcap));
  if ((reinterpret_cast<uintptr_t>(prompt_h) | reinterpret_cast<uintptr_t>(prompt_feat)) & 15)
    return fail(JV_ERR_ARG, "jv_cfm_pool_admit: prompt_h / prompt_feat must be 16-byte aligned");
  const int Pmax = std::min(Ph, Pf);
  std::vector<char> seen((size_t)slots, 0);
  int tmax = 0;
  char msg[200];
  for (int b = 0; b < B; ++b) {
    const int y = h_ylens[b], p = h_plens[b];
    if (p < 0 || p > Pmax) {
      snprintf(msg, sizeof msg, "%s: request %d: prompt length %d outside [0, min(Ph, Pf) = %d]", who, b, p, Pmax);
      return fail(JV_ERR_ARG, msg);
    }
    if (y < 0 || y > Ty) {
      snprintf(msg, sizeof msg, "%s: request %d: %d frames outside [0, Ty = %d]", who, b, y, Ty);
      return fail(JV_ERR_ARG, msg);
    }
    if (p + y < 1 || p + y > Tcap || p + y > NOISE_FRAMES) {
      snprintf(msg, sizeof msg, "%s: request %d: %d + %d frames outside [1, min(Tcap = %d, %d)]", who, b, p, y, Tcap, NOISE_FRAMES);
      return fail(JV_ERR_ARG, msg);
    }
    if (!(h_temps[b] == h_temps[b])) {
      snprintf(msg, sizeof msg, "%s: request %d: temperature is not a number", who, b);
      return fail(JV_ERR_ARG, msg);
    }
    JV_TRY(pool_check_slot(who, b, h_slots[b], slots, seen));
    tmax = std::max(tmax, p + y);
  }
  for (int b0 = 0; b0 < B; b0 += POOL_CHUNK) {
    PoolAdmitChunk ch;
    ch.n = std::min(POOL_CHUNK, B - b0); ch.b0 = b0;
    int cmax = 0;
    for (int i = 0; i < ch.n; ++i) {
      ch.r[i] = {h_slots[b0 + i], h_plens[b0 + i], h_plens[b0 + i] + h_ylens[b0 + i], h_temps[b0 + i]};
      cmax = std::max(cmax, ch.r[i].len);
    }
    for (int i = ch.n; i < POOL_CHUNK; ++i) ch.r[i] = {0, 0, 0, 0.f};
    JV_TRY(pool_admit(ch, cmax, mu_y, Ty, prompt_h, Ph, prompt_feat, Pf, spks, c.noise, NOISE_FRAMES, pool_x, pool_mu, pool_cond,
                      pool_spks, pool_amax, Tcap, st));
  }
  (void)tmax;
  return JV_OK;
}

int cfm_pool_step(Context& c, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks, float* pool_amax,
                  int slots, int Tcap, const int* h_slots, const int* h_lens, const float* h_t, const float* h_dt, int B,
                  hipStream_t st, const float* h_cfg, const int* h_stage, float* pool_x0, float* pool_k1) {
  const char* who = h_stage ? "jv_cfm_pool_step_s" : h_cfg ? "jv_cfm_pool_step_g" : "jv_cfm_pool_step";
  if (!c.ready[MODEL_FLOW]) return fail(JV_ERR_STATE, "tts weights not finalized");
  JV_TRY(pool_check_pools(who, pool_x, pool_mu, pool_cond, pool_spks, nullptr, slots, Tcap));
  if (h_stage) JV_TRY(pool_check_pools(who, pool_x0, pool_k1, nullptr, nullptr, nullptr, slots, Tcap));
  FlowWs& w = *c.flow;
  char msg[200];
  if (B < 1 || B > c.max_batch) {
    snprintf(msg, sizeof msg, "%s: %d requests outside [1, max_batch = %d]: beyond the reservation (jv_reserve)", who, B, c.max_batch);
    return fail(B < 1 ? JV_ERR_ARG : JV_ERR_SHAPE, msg);
  }
  std::vector<char> seen((size_t)slots, 0);
  int T = 0;
  for (int b = 0; b < B; ++b) {
    JV_TRY(pool_check_slot(who, b, h_slots[b], slots, seen));
    if (h_lens[b] < 1 || h_lens[b] > Tcap) {
      snprintf(msg, sizeof msg, "%s: request %d: %d frames outside [1, Tcap = %d]", who, b, h_lens[b], Tcap);
      return fail(JV_ERR_ARG, msg);
    }
    if (h_lens[b] > c.max_frames) {
      snprintf(msg, sizeof msg, "%s: request %d: %d frames exceed the reservation (max_frames = %d)", who, b, h_lens[b], c.max_frames);
      return fail(JV_ERR_SHAPE, msg);
    }
    if (!(h_t[b] == h_t[b]) || !(h_dt[b] == h_dt[b])) {
      snprintf(msg, sizeof msg, "%s: request %d: t / dt is not a number", who, b);
      return fail(JV_ERR_ARG, msg);
    }
    if (h_cfg && !guidance_rate_ok(h_cfg[b])) {
      snprintf(msg, sizeof msg, "%s: request %d: guidance rate %g must be finite and >= 0", who, b, (double)h_cfg[b]);
      return fail(JV_ERR_ARG, msg);
    }
    if (h_stage) {      // a stage of the request's own solver (jv_ops.h STAGE_*), and the pools that stage saves to or reads from
      if (!stage_ok(h_stage[b])) {
        snprintf(msg, sizeof msg, "%s: request %d: stage %d is none of JV_STAGE_EULER, _MID1, _MID2, _HEUN1, _HEUN2", who, b, h_stage[b]);
        return fail(JV_ERR_ARG, msg);
      }
      if ((h_stage[b] != STAGE_EULER && !pool_x0) || ((h_stage[b] & (STAGE_SAVE_K1 | STAGE_ADD_K1)) && !pool_k1)) {
        snprintf(msg, sizeof msg, "%s: request %d: stage %d saves to or reads from pool_x0 / pool_k1, which is null", who, b, h_stage[b]);
        return fail(JV_ERR_ARG, msg);
      }
    }
    T = std::max(T, h_lens[b]);
  }
  // the step's rows, by cfm_solve's rule: compact where the route allows it and it saves rows, else uniform (padded to T)
  const int B2 = 2 * B;
  Geo g{B2, T, T + FLOW_GAP, flow_rows(B2, T), w.rows_alloc, w.t_dev, 1};
  std::vector<int> uoff((size_t)B2 + 1);
  long r = 0, frames = 0;
  const bool compact = B > 1 && flow_compact_ok(c, g.M) && compact_plan(c, g.M, h_lens, B, B2, T, uoff.data(), &r, &frames);
  if (compact) { g.M = r; g.uoff = w.uoff; g.alg_rows = frames; }
  if (g.M + 128 > w.rows_alloc) {      // (implied by the two limits above: the workspace holds 2 max_batch padded utterances)
    snprintf(msg, sizeof msg, "%s: request %d: the step's %ld rows exceed the reservation (%ld)", who, B - 1, g.M, w.rows_alloc - 128);
    return fail(JV_ERR_SHAPE, msg);
  }
  // ---- nothing was launched up to here ----
  for (int b0 = 0; b0 < B; b0 += POOL_CHUNK) {
    PoolStepChunk ch;
    ch.n = std::min(POOL_CHUNK, B - b0); ch.b0 = b0;
    for (int i = 0; i < POOL_CHUNK; ++i) {
      const int b = b0 + i;
      if (i < ch.n)
        ch.r[i] = {h_slots[b], h_lens[b], compact ? uoff[b] : FLOW_G + b * g.S, compact ? uoff[B + b] : FLOW_G + (B + b) * g.S, h_t[b], h_dt[b],
                   h_cfg ? h_cfg[b] : 0.7f, h_stage ? h_stage[b] : STAGE_EULER};
      else
        ch.r[i] = {0, 0, 0, 0, 0.f, 0.f, 0.f, STAGE_EULER};
    }
    JV_TRY(pool_publish(ch, B, w.pool_req, w.lens2, w.t_dev, compact ? w.uoff : nullptr, (int)g.M, st));
  }
  JV_TRY(row_meta(w.rowmask, w.row_sample, w.lens2, B2, 1, FLOW_G, g.S, T, w.rows_alloc, 1, 0, st, g.uoff));
  JV_TRY(pool_gather(w.pool_req, B, T, compact ? 0 : T, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, Tcap, w.x, w.mu, w.cond,
                     w.spks, w.amax, w.amax_stride, st));
  JV_TRY(assemble_xin(w.x, w.mu, w.spks, w.cond, w.xin, B, B, FLOW_G, g.S, T, g.M, st, g.uoff, w.row_sample, w.rowmask));
  JV_TRY(estimator_body(c, g, est_route(c, g.M, /*temb_pre=*/false, compact, c.attn_chunk), st));
  // (two rows per frame for every request, one at rate 0 included: its twin is computed and (1 + 0) d_c - 0 d_u = d_c)
  if (h_stage) return pool_stage_scatter(w.pool_req, B, T, w.x, w.d, w.amax, w.amax_stride, pool_x, pool_x0, pool_k1, pool_amax, Tcap, st);
  return pool_euler_scatter(w.pool_req, B, T, w.x, w.d, w.amax, w.amax_stride, pool_x, pool_amax, Tcap, st);
}

int cfm_pool_fetch(Context& c, const float* pool_x, int slots, int Tcap, const int* h_slots, const int* h_first, const int* h_lens,
                   int B, int Tm, float* mel, hipStream_t st) {
  (void)c;
  const char* who = "jv_cfm_pool_fetch";
  if (B < 1 || Tm < 1 || slots < 1 || Tcap < 1) return fail(JV_ERR_ARG, "jv_cfm_pool_fetch: B, Tm, slots and Tcap must be positive");
  char msg[200];
  for (int b = 0; b < B; ++b) {
    if (h_slots[b] < 0 || h_slots[b] >= slots) {
      snprintf(msg, sizeof msg, "%s: request %d: slot %d outside [0, %d)", who, b, h_slots[b], slots);
      return fail(JV_ERR_ARG, msg);
    }
    if (h_first[b] < 0 || h_lens[b] < 0 || h_lens[b] > Tm || (long)h_first[b] + h_lens[b] > Tcap) {
      snprintf(msg, sizeof msg, "%s: request %d: frames [%d, %d + %d) outside the slot (Tcap = %d) or longer than Tm = %d", who, b,
               h_first[b], h_first[b], h_lens[b], Tcap, Tm);
      return fail(JV_ERR_ARG, msg);
    }
  }
  for (int b0 = 0; b0 < B; b0 += POOL_CHUNK) {
    PoolFetchChunk ch;
    ch.n = std::min(POOL_CHUNK, B - b0); ch.b0 = b0;
    for (int i = 0; i < POOL_CHUNK; ++i)
      ch.r[i] = i < ch.n ? PoolFetchReq{h_slots[b0 + i], h_first[b0 + i], h_lens[b0 + i]} : PoolFetchReq{0, 0, 0};
    JV_TRY(pool_fetch(ch, pool_x, Tcap, mel, Tm, st));
  }
  return JV_OK;
}

constexpr int T2M_EST_CHUNK = 50;     // the estimator's static_chunk_size in frames (configs/base.yaml:98; decoder.py:951-954)

// Token-to-mel (flow/flow.py:314-358 looped over the utterances): the flow encoder's h over [prompt tokens | tokens] is mu for the
// whole sequence of T_b = 2 (p_b + n_b) frames, cond = [prompt_feat_b[:f_b] | 0], and frames f_b .. T_b - 1 come back.  The same
// schedule, geometry rule, Euler loop, pack and unpack kernels as cfm_solve_prompted: in its terms every frame is a "prompt" frame
// of mu (Ty = 0) and the condition prefix has a length of its own.
// ctx = 3 (jv_flow_token2mel_partial; flow.py:327-336): the last three tokens are look-ahead context of the encoder only, so the
// sequence is L = P + N - 3 tokens and everything from h onwards -- lengths, masks, the solve, the unpack -- runs on 2 L frames.
// ctx_lens (jv_flow_token2mel_ctx; ctx = 0): a context per utterance, 0 or 3 tokens.  Utterance b runs on L_b = p_b + n_b - ctx_b
// tokens in buffers of the whole sequence's width, Tm = 2 (P + N).  Its lengths come down FIRST and are checked before anything
// is launched on them (flow_ctx_lengths): that is the call's one synchronisation, and the f_b come down with it.
int flow_token2mel(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, const float* prompt_feat,
                   const int* feat_lens, const float* embedding, int B, int P, int N, int F, int streaming, int n_timesteps,
                   float temperature, const float* t_span_host, float* mel, int* mel_lens, hipStream_t st, int ctx,
                   const int* ctx_lens) {
  if (!c.ready[MODEL_FLOW]) return fail(JV_ERR_STATE, "flow decoder weights not finalized (JV_MODEL_FLOW or JV_MODEL_TTS)");
  if (!c.ready[MODEL_PROMPT]) return fail(JV_ERR_STATE, "prompt encoder weights not finalized");
  if (B < 1 || P < 0 || N < 0 || P + N < 1 || F < 0) return fail(JV_ERR_ARG, "jv_flow_token2mel: B, P + N must be positive, P, N, F non-negative");
  if (B > c.max_batch) return fail(JV_ERR_SHAPE, "batch/frames exceed the capacity given to jv_create");
  if (!c.noise_loaded) return fail(JV_ERR_STATE, "CFM noise tensor not loaded (jv_load_noise)");
  FlowWs& w = *c.flow;
  if (n_timesteps < 1 || n_timesteps > w.max_steps) return fail(JV_ERR_ARG, "n_timesteps out of range");
  if (reinterpret_cast<uintptr_t>(prompt_feat) & 15) return fail(JV_ERR_ARG, "jv_flow_token2mel: prompt_feat must be 16-byte aligned");
  if (ctx < 0 || P + N - ctx < 1) return fail(JV_ERR_ARG, "jv_flow_token2mel_partial: P + N must be at least 4 (one encoded token + 3 of context)");
  JV_TRY(guidance_check(c, "jv_flow_token2mel", n_timesteps));
  JV_TRY(solver_check(c, "jv_flow_token2mel", n_timesteps));
  const int B2 = solve_twins(c, n_timesteps) ? 2 * B : B, Tm = 2 * (P + N - ctx);
  JV_TRY(check_shape(c, 2 * B, Tm));
  if (Tm > NOISE_FRAMES) return fail(JV_ERR_SHAPE, "more frames than the fixed noise tensor holds (15000)");

  // h [B, Tm, 80] and the projected speaker vectors wait in buffers the estimator writes only once the loop runs: w.d (its
  // output, rows_alloc * 80 floats >= B * Tm * 80) and w.tsin ([2B, 320]); solve_loop copies the vectors to w.spks first
  float* const h = w.d;
  float* const spks = w.tsin;
  int* const hl = w.t2m_lens;
  int* const yl = w.t2m_lens + c.max_batch;
  std::vector<float> tt, dts;
  if (ctx_lens) {
    if (ctx != 0) return fail(JV_ERR_ARG, "jv_flow_token2mel_ctx: one context for the call or one per utterance, not both");
    std::vector<int> enc_lens, f_host;
    JV_TRY(solve_schedule(c, w, n_timesteps, t_span_host, tt, dts, st));
    JV_TRY(flow_ctx_lengths("jv_flow_token2mel_ctx", plen, len, ctx_lens, feat_lens, B, P, N, enc_lens, &f_host, st));
    for (int b = 0; b < B; ++b) {
      w.h_lens[b] = 2 * enc_lens[b];
      w.h_lens[B + b] = f_host[b];
    }
    JV_TRY(flow_encoder_fwd_ctx(c, ptok, plen, tok, len, ctx_lens, B, P, N, streaming, h, hl, st, true));
    JV_TRY(speaker_projection(c, embedding, B, spks, st));
  } else {
    JV_TRY(flow_encoder_fwd(c, ptok, plen, tok, len, B, P, N, streaming, h, hl, st, ctx));
    JV_TRY(speaker_projection(c, embedding, B, spks, st));

    JV_TRY(solve_schedule(c, w, n_timesteps, t_span_host, tt, dts, st));
    JV_HIP(hipMemcpyAsync(w.h_lens, hl, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    JV_HIP(hipMemcpyAsync(w.h_lens + B, feat_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    JV_HIP(hipStreamSynchronize(st));
  }
  int T = 0;
  for (int b = 0; b < B; ++b) {
    const int tb = w.h_lens[b], f = w.h_lens[B + b];
    if (f < 0 || f > std::min(F, tb)) {
      char msg[200];
      snprintf(msg, sizeof msg, "jv_flow_token2mel: utterance %d: prompt_feat length %d outside [0, min(F = %d, 2 * tokens = %d)]", b, f, F, tb);
      return fail(JV_ERR_ARG, msg);
    }
    w.h_sum[b] = w.h_sum[B + b] = tb;
    w.h_y[b] = tb - f;
    T = std::max(T, tb);
  }
  if (T < 1) {      // every utterance empty: nothing to solve
    JV_HIP(hipMemsetAsync(mel, 0, sizeof(float) * 80 * (size_t)B * Tm, st));
    if (mel_lens) JV_HIP(hipMemsetAsync(mel_lens, 0, sizeof(int) * B, st));
    return JV_OK;
  }
  Geo g{B2, T, T + FLOW_GAP, flow_rows(B2, T), w.rows_alloc, nullptr, 0};
  if (B > 1 && flow_compact_ok(c, g.M)) JV_TRY(solve_compact(c, g, w.h_sum, B, T, st));

  JV_HIP(hipMemcpyAsync(w.lens2, w.h_sum, sizeof(int) * B2, hipMemcpyHostToDevice, st));      // (pinned: stays valid)
  JV_HIP(hipMemcpyAsync(yl, w.h_y, sizeof(int) * B, hipMemcpyHostToDevice, st));
  const int* const clens = g.uoff ? w.lens2 : nullptr;
  JV_TRY(row_meta(w.rowmask, w.row_sample, w.lens2, B2, 1, FLOW_G, g.S, T, w.rows_alloc, 1, 0, st, g.uoff));
  JV_TRY(pack_prompted(nullptr, 0, h, Tm, prompt_feat, F, hl, w.lens2, B, T, w.mu, w.cond, FLOW_G, g.S, st, g.uoff, feat_lens));
  JV_TRY(cf_to_rows(c.noise, 0, NOISE_FRAMES, B, 80, T, w.x, 80, 0, FLOW_G, g.S, temperature, clens, st, g.uoff));

  const int chunk_was = c.attn_chunk;
  c.attn_chunk = streaming ? T2M_EST_CHUNK : 0;
  const int rc = solve_loop(c, g, spks, B, T, n_timesteps, lens_all_equal(w.h_sum, B, T), st);
  c.attn_chunk = chunk_was;
  JV_TRY(rc);
  if (mel_lens) JV_HIP(hipMemcpyAsync(mel_lens, yl, sizeof(int) * B, hipMemcpyDeviceToDevice, st));
  return rows_to_cf_from(w.x, 80, FLOW_G, g.S, feat_lens, yl, mel, 80L * Tm, B, 80, Tm, st, g.uoff);
}

void flow_ws_destroy(Context& c) {
  if (c.flow) {
    flow_graphs_drop(c);
    if (c.flow->gstream) (void)hipStreamDestroy(c.flow->gstream);
    if (c.flow->ev_in) (void)hipEventDestroy(c.flow->ev_in);
    if (c.flow->ev_out) (void)hipEventDestroy(c.flow->ev_out);
    if (c.flow->h_lens) (void)hipHostFree(c.flow->h_lens);
    if (c.flow->h_uoff) (void)hipHostFree(c.flow->h_uoff);
    if (c.flow->h_sum) (void)hipHostFree(c.flow->h_sum);
    if (c.flow->h_y) (void)hipHostFree(c.flow->h_y);
  }
  delete c.flow;
  c.flow = nullptr;
}
}  // namespace jv
