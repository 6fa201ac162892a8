// Declarations of the small row-buffer kernels (rowops.hip, hiftops.hip, encops.hip).
#pragma once
#include "jv_common.h"

namespace jv {

// uoff (optional, [nb * reps + 1] first rows, device): the COMPACT geometry of ragged batches -- utterance b at rows uoff[b] ..,
// no padding to the longest (rowops.hip); null: the uniform geometry G + b S + t
int row_meta(unsigned char* rowmask, int* row_sample, const int* lens, int nb, int reps, int G, int S, int L, long rows,
             int mul, int add, hipStream_t st, const int* uoff = nullptr);
// dst[i] = min(max(src[i % nb], 0), T), i < nb * reps: the entry points' length contract (jyutvoice_hip.h "Lengths")
int clamp_lens(const int* src, int nb, int reps, int T, int* dst, hipStream_t st);
// src[b*src_bstride + c*pitch + t] (channels-first) -> dst[(G + b*S + t)*ld + col0 + c]
int cf_to_rows(const float* src, long src_bstride, long pitch, int B, int C, int T, float* dst, int ld, int col0, int G,
               int S, float scale, const int* lens, hipStream_t st, const int* uoff = nullptr);
// (the inverse; positions at and behind min(lens[b] * len_mul + len_add, T) are written as zeros)
int rows_to_cf(const float* src, int ld, int col0, int G, int S, float* dst, long dst_bstride, int B, int C, int T,
               const int* lens, hipStream_t st, const int* uoff = nullptr, int len_mul = 1, int len_add = 0);
// cfm_solve_prompted's pack and unpack (rowops.hip): row-layout mu / cond of [prompt_b | text_b] sequences in one launch; the
// generated frames first[b] .. first[b] + lens[b] - 1 back to channels-first, zero-filled to T.  clens (optional): the condition
// prefix has a length of its own, cond = [prompt_feat_b[:clens[b]] | 0] while mu = [prompt_h[b, :plens[b]] | mu_y] (token-to-mel:
// all of mu comes from the flow encoder, plens = sums, Ty = 0); null: clens = plens
int pack_prompted(const float* mu_y, int Ty, const float* prompt_h, int Ph, const float* prompt_feat, int Pf, const int* plens,
                  const int* sums, int B, int T, float* mu, float* cond, int G, int S, hipStream_t st, const int* uoff = nullptr,
                  const int* clens = nullptr);
int rows_to_cf_from(const float* src, int ld, int G, int S, const int* first, const int* lens, float* dst, long dst_bstride,
                    int B, int C, int T, hipStream_t st, const int* uoff = nullptr);
// ntwin: the unconditional twin slots to fill behind the B conditional ones (B; 1: the twin a solve's first step shares; 0: none)
int assemble_xin(const float* x, const float* mu, const float* spks, const float* cond, float* xin, int B, int ntwin, int G,
                 int S, int L, long rows2, hipStream_t st, const int* uoff = nullptr, const int* row_sample = nullptr,
                 const unsigned char* rowmask = nullptr);
int assemble_xin_plain(const float* x, const float* mu, const float* spks, const float* cond, float* xin, int B, int G,
                       int S, int L, long rows, hipStream_t st);
void time_freq_table(float* f);      // [160], host: the sinusoid's frequencies, correctly rounded
int time_sinusoid(const float* t, int t_stride, const float* freq, float* out, int B, hipStream_t st);      // freq: that table on the device
// rate: the step's guidance rate, one float on the device.  one_twin: every utterance reads the twin at slot B.  no_twin: the
// step of rate 0 on B utterances alone, x += dt d (rate is not read, no twin row is addressed)
int euler_cfg(float* x, const float* d, int B, int G, int S, int L, const float* dt_table, int step, const float* rate,
              hipStream_t st, const int* uoff = nullptr, const int* lens = nullptr, bool one_twin = false, bool no_twin = false);
// One stage of a second-order CFM step (flow.hip solve_loop; DESIGN.md 5 "Solver"), with g = (1 + r) d_cond - r d_uncond as euler_cfg
// forms it (twin: SOLVER_TWIN_*; none: g = d_cond, no twin row is addressed) and c = coef[0], the stage's coefficient:
//   base = stage & STAGE_BASE_X0 ? x0 : x;   inc = stage & STAGE_ADD_K1 ? k1 + g : g;   x <- base + c inc
// and before that x0 <- x (STAGE_SAVE_X0), k1 <- g (STAGE_SAVE_K1).  x afterwards is the estimator's next input.
//   midpoint: STAGE_MID1 with c = 0.5f dt (xs = x + c g, x0 kept), then STAGE_MID2 with c = dt (x = x0 + c g(xs))
//   Heun:     STAGE_HEUN1 with c = dt (k1 = g, xs = x + c k1), then STAGE_HEUN2 with c = 0.5f dt (x = x0 + c (k1 + g(xs)))
// STAGE_EULER (0, c = dt) is euler_cfg's update.  Also the stage codes of PoolStepReq::stage and jv_cfm_pool_step_s.
constexpr int STAGE_SAVE_X0 = 1, STAGE_SAVE_K1 = 2, STAGE_BASE_X0 = 4, STAGE_ADD_K1 = 8;
constexpr int STAGE_EULER = 0, STAGE_MID1 = STAGE_SAVE_X0, STAGE_MID2 = STAGE_BASE_X0, STAGE_HEUN1 = STAGE_SAVE_X0 | STAGE_SAVE_K1,
              STAGE_HEUN2 = STAGE_BASE_X0 | STAGE_ADD_K1;
inline bool stage_ok(int s) { return s == STAGE_EULER || s == STAGE_MID1 || s == STAGE_MID2 || s == STAGE_HEUN1 || s == STAGE_HEUN2; }
constexpr int SOLVER_TWIN_NONE = 0, SOLVER_TWIN_SHARED = 1, SOLVER_TWIN_EACH = 2;      // shared: every utterance reads the twin at slot B
int solver_stage(float* x, float* x0, float* k1, const float* d, int B, int G, int S, int L, const float* coef, const float* rate,
                 int stage, int twin, hipStream_t st, const int* uoff = nullptr, const int* lens = nullptr);
int ln_epilogue_rows(float* x, const float* g, const float* b, float eps, long rows, int C, int act,
                     const unsigned char* rowmask, const float* rowvec, const int* row_sample, int rowvec_ld, const float* res,
                     long ldr, float scale, hipStream_t st, float* amax_out = nullptr, int amax_G = 0, int amax_S = 0,
                     int amax_nb = 1, const int* amax_rows = nullptr);
// cfmpool.hip: in-flight batching (flow.hip cfm_pool_*).  A request's solver state lives in caller-owned pools, [slots, Tcap, 80]
// frame-major x / mu / cond, [slots, 80] spks, [slots, 3, 2] running trunk maxima (buffer; request, CFG twin).  What the host
// decides per call travels as kernel ARGUMENTS, POOL_CHUNK requests per launch: a launch snapshots its arguments, so a call needs
// neither a synchronisation nor a staging buffer that the next call could rewrite under a copy still queued.
constexpr int POOL_CHUNK = 64;
struct PoolAdmitReq { int slot, p, len; float temp; };      // prompt frames, p + y frames, noise scale
struct PoolAdmitChunk { int n, b0; PoolAdmitReq r[POOL_CHUNK]; };
// first workspace row of the request and of its CFG twin; its guidance rate in this step; stage: STAGE_* above, of which dt is the
// coefficient (jv_cfm_pool_step / _g: STAGE_EULER and the step's dt)
struct PoolStepReq { int slot, len, row, rowu; float t, dt, cfg; int stage; };
struct PoolStepChunk { int n, b0; PoolStepReq r[POOL_CHUNK]; };
struct PoolFetchReq { int slot, first, len; };
struct PoolFetchChunk { int n, b0; PoolFetchReq r[POOL_CHUNK]; };
// mu = [prompt_h[b, :p] | mu_y[b, :, :len - p]], cond = [prompt_feat[b, :p] | 0], x = noise[:, :len] * temp, spks, maxima = 0
int pool_admit(const PoolAdmitChunk& ch, int tmax, const float* mu_y, int Ty, const float* prompt_h, int Ph, const float* prompt_feat,
               int Pf, const float* spks, const float* noise, long noise_pitch, float* pool_x, float* pool_mu, float* pool_cond,
               float* pool_spks, float* pool_amax, int Tcap, hipStream_t st);
// the step's tables from the arguments: req[b], lens2[b] = lens2[B + b] = len, t_dev[b] = t_dev[B + b] = t and, with uoff (compact
// geometry), uoff[b] = row, uoff[B + b] = rowu, uoff[2B] = rows_end
int pool_publish(const PoolStepChunk& ch, int B, PoolStepReq* req, int* lens2, float* t_dev, int* uoff, int rows_end, hipStream_t st);
// pools -> workspace rows of the B requests (x, mu, cond; zeros for frames len .. tfill - 1: the uniform geometry's padding), their
// spks and the maxima of request and twin into amax[k * amax_stride + b] / [.. + B + b]
int pool_gather(const PoolStepReq* req, int B, int tmax, int tfill, const float* pool_x, const float* pool_mu, const float* pool_cond,
                const float* pool_spks, const float* pool_amax, int Tcap, float* x, float* mu, float* cond, float* spks, float* amax,
                int amax_stride, hipStream_t st);
// pool_x[slot, t] = x[row + t] + dt_b ((1 + cfg_b) d[row + t] - cfg_b d[rowu + t]) (euler_cfg with a dt and a rate per request), maxima back
int pool_euler_scatter(const PoolStepReq* req, int B, int tmax, const float* x, const float* d, const float* amax,
                       int amax_stride, float* pool_x, float* pool_amax, int Tcap, hipStream_t st);
// pool_euler_scatter's stage-aware sibling (jv_cfm_pool_step_s): solver_stage per request, stage and coefficient from req[b], on
// the caller's pools -- base and the saved k1 are read from pool_x0 / pool_k1, x0 <- the step's input (x[row + t], what pool_x held)
// and k1 <- g are saved there, and pool_x takes the estimator's next input (xs or the new x), so the gather is pool_gather for
// every stage.  pool_x0 / pool_k1 may be null where no listed stage touches them (checked by the caller)
int pool_stage_scatter(const PoolStepReq* req, int B, int tmax, const float* x, const float* d, const float* amax, int amax_stride,
                       float* pool_x, float* pool_x0, float* pool_k1, float* pool_amax, int Tcap, hipStream_t st);
// mel[b, c, t] = pool_x[slot, first + t, c] for t < len, zeros up to Tm
int pool_fetch(const PoolFetchChunk& ch, const float* pool_x, int Tcap, float* mel, int Tm, hipStream_t st);

int fill(float* p, float v, long n, hipStream_t st);
int fill_int(int* p, int v, long n, hipStream_t st);

}  // namespace jv
