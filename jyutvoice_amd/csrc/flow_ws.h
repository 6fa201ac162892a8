// What flow.hip (workspace, entry points, solver) and estimator.hip (one estimator evaluation) share: the workspace, the row
// geometry of a call, the route record, and the host launchers of rowgemm.hip / rowblock.hip.
#pragma once
#include <vector>
#include "jv_model.h"
#include "jv_ops.h"
#include "rowblock_kernel.h"
#include "rowconv_kernel.h"
#include "rowres_kernel.h"

namespace jv {

// rowgemm.hip
int rowgemm(const RowGemmArgs& a, int epi, hipStream_t st);
int rowconv(const RowConvArgs& a, hipStream_t st);
int rowres(const RowResArgs& a, hipStream_t st);      // a whole resnet in one launch
bool rowres_fits(int M);
bool rowconv_w_direct(const RowConvArgs& a);
int rowffn(const RowFfnArgs& a, hipStream_t st);
int rowgemm_tile(int M);
int rowblock(const RowBlockArgs& a, bool qkv, hipStream_t st);      // rowblock.hip

constexpr int FLOW_G = 4;      // leading guard rows (>= causal left context 2)
constexpr int FLOW_GAP = 4;    // rows between utterances
constexpr int PARTIAL_ROWS = 2048, PARTIAL_SPLITS = 8;      // split-K is for short M only (est_route)
constexpr int TS_MAX = 64;      // evaluations whose timestep embeddings cfm_solve computes ahead of the loop (more: per evaluation, as the seam does)

struct FlowWs {
  long rows_alloc = 0;      // rows every [*,C] buffer below can hold
  float *x = nullptr, *mu = nullptr, *cond = nullptr, *spks = nullptr;   // [rows,80] x3, [maxB,80]
  // second-order solves (jv_flow_set_solver; flow.hip solve_loop): the state x0 a step started from (midpoint, Heun) and its first
  // slope k1 (Heun), saved by the first stage for the second while x holds the stage point xs; [rows,80] each, untouched by Euler
  float *x0 = nullptr, *k1 = nullptr;
  float *xin = nullptr;                                               // [rows,320]
  float *h = nullptr, *h2 = nullptr, *res = nullptr, *cat = nullptr;  // [rows,256] x3, [rows,512]
  float *ln = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr; // 256, 1536, 512, 1024
  // max |value| written to the trunk buffers during the current solve, one slot per BUFFER (h, h2, cat: a launch never
  // reads the slot it writes) and per UTTERANCE (CFG twins count as utterances of their own: [3][2 * max_batch] floats):
  // every kernel that writes one of them tracks it (ConvGemmArgs::amax_out, ln_epilogue_rows), and the convolutions that
  // read them -- whose input, the residual stream, has no load-time bound -- derive their fp16x3 scale from it (amax_in).
  // An utterance's scales therefore depend on that utterance alone: its result is the same bit for bit whatever else is
  // in the batch and however a batch is sharded over GPUs.  Zeroed once per solve.
  float* amax = nullptr;
  int amax_stride = 0;      // floats per buffer = 2 * max_batch
  float* partial = nullptr;      // [8][PARTIAL_ROWS][256] split-K partial sums (short M only)
  unsigned long long* rb_stamps = nullptr;      // tuning builds, JV_RB_STAMPS: rowblock_kernel's phase stamps of the last launch
  unsigned long long* rc_stamps = nullptr;      // ... and rowconv_wd_kernel's
  float *d = nullptr;                                                 // [rows,80]
  float *tsin = nullptr, *t1 = nullptr, *tmish = nullptr, *temb = nullptr;
  float* tfreq = nullptr;      // [160] the sinusoid's fp32 frequency table (time_freq_table)
  float *t_dev = nullptr, *t_table = nullptr, *dt_table = nullptr;
  // (t_table, dt_table, cfg_table hold one entry per estimator EVALUATION: an Euler step is one, a midpoint / Heun step two, and
  // dt_table holds the coefficient of the evaluation's update -- dt, or 0.5f dt in a half stage; solve_schedule)
  float *cfg_table = nullptr;      // the guidance rate of every evaluation of the solve, [max_steps] (jv_flow_set_guidance; solve_schedule)
  // cfm_solve: the timestep embedding of EVERY step of a solve, computed in three launches before the loop (the steps'
  // t are known up front and the same for all rows): [TS_MAX] rows of sinusoid / hidden / Mish / the 14 projections
  float *ts_sin = nullptr, *ts_1 = nullptr, *ts_mish = nullptr, *ts_emb = nullptr;
  unsigned char* rowmask = nullptr;
  int* row_sample = nullptr;
  int* lens2 = nullptr;     // [2*maxB]
  // COMPACT geometry of ragged batches (cfm_solve): first row of every utterance (+ the first row past the batch), [2*maxB + 1];
  // h_lens / h_uoff: pinned host staging (the lengths come down with the solve's one synchronisation, the offsets go up async)
  int* uoff = nullptr;
  int *h_lens = nullptr, *h_uoff = nullptr;
  int* h_sum = nullptr;     // cfm_solve_prompted: p_b + y_b of every utterance and its CFG twin, [2*maxB] (pinned; goes up to lens2)
  int* t2m_lens = nullptr;  // flow_token2mel: T_b = 2 (p_b + n_b) in [0, maxB), y_b = T_b - f_b in [maxB, 2*maxB) (device)
  int* h_y = nullptr;       // ... and y_b on its way up, [maxB] (pinned)
  PoolStepReq* pool_req = nullptr;      // cfm_pool_step: the step's requests (slot, length, rows, t, dt, guidance rate), [maxB] (device; cfmpool.hip)
  int max_steps = 1024;      // estimator evaluations of one solve (the tables' length): n_timesteps, twice that for a second-order solver
  // One Euler step (step scalars -> input assembly -> estimator -> CFG update) captured as a hipGraph per (B, T,
  // attention mode): the step reads its (t, dt, guidance rate) through a device-side counter, so one executable graph replays
  // for every step of every solve of that geometry -- a solve with a step WITHOUT twins (rate 0) never replays it, it is eager.  Replayed on a private stream (the caller's may be the legacy
  // default stream, which cannot be captured), fenced against the caller's stream with events.
  int* step_ctr = nullptr;
  float *t_cur = nullptr, *dt_cur = nullptr, *cfg_cur = nullptr;      // (t, dt, guidance rate) of the running step (step_advance_kernel)
  struct StepGraph { int B, T, chunk, pre; hipGraph_t graph; hipGraphExec_t exec; };      // pre: captured with the embeddings precomputed
  std::vector<StepGraph> graphs;
  hipStream_t gstream = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
};

struct Geo {
  int B2, T, S;
  long M;        // rows computed by every GEMM: [0, M)
  long a_rows;   // rows that may be read
  const float* t_ptr = nullptr;   // timestep per utterance: t_ptr[b * t_stride]
  int t_stride = 1;
  bool temb_pre = false;          // w.temb row 0 already holds this step's embedding, the same for every utterance (cfm_solve)
  // COMPACT geometry (ragged batches, cfm_solve): utterance b starts at row uoff[b] and owns lens2[b] rows + the gap; M is then
  // G + sum (len + gap), not G + B2 (T + gap), and every launch of the call is that much shorter.  null: uniform, G + b S + t
  const int* uoff = nullptr;
  long alg_rows = 0;              // profiler: real frames of the call (0: B2 * T)
  long frames() const { return alg_rows ? alg_rows : (long)B2 * T; }
};

// Which of the estimator's regimes every launch of a call belongs to: decided once per call / per solve by est_route() from the
// mode switches (Context), the row count and the load-time weight bits (BtbW / ResnetW / EstimatorW), and read -- never
// re-derived -- by everything that launches (estimator.hip) or lays rows out (flow.hip).  DESIGN.md 5 "Estimator routes".
// a resnet: on the tile kernels (block1, res_conv, block2; the two split K at short M) / on the row-owning convolutions wherever
// the input has a tracked bound (block1 + res_conv, block2) / as one launch that never writes the buffer it reads (rowres_kernel.h)
enum ResRoute : int { RES_TILES, RES_ROWS, RES_ONE };
struct EstRoute {
  bool exact = false;        // bf16x6 everywhere: no fp16x3 operands, no bound tracking
  int np = 3;                // products per step of every fp16x3 contraction of the call: 3, or 1 = hi x hi alone (Context::est_fp16); Est hands it to every launcher
  bool attn_single = true;   // row-owning stages: attention_s.hip where the batch fills its rounds; false (np = 1: that kernel writes its three terms out as asm) always attention_pl.hip
  bool rows = false;         // the batch fills the chip: row-owning kernels (else the tile kernels)
  int ksplit = 1;            // > 1: short M, K split over this many workgroups per tile
  bool sk_blocks = false;    // every block's to_out / ff.net.2 splits K and its reduce tail writes the next LayerNorm
  bool pre_planes = false;   // tile route: fp16x3 linears take their A operand pre-split from the producer (JV_DMA_A)
  int qkv_split = 1, qkv_rt = 0;      // > 1: q | k | v leaves the fused block, its column chunks dealt over qkv_split workgroups per 16 * qkv_rt rows
  bool ffn_fuse = true;      // row-owning blocks: the feed-forward pair in one launch (rowffn_kernel) ...
  bool block_fuse = true;    // ... with to_out and the next block's q | k | v too (rowblock_kernel.h), where the weights allow
  int attn_chunk = 0;        // > 0: streaming (chunk-causal) attention, in frames
  bool compact = false;      // the call's rows are laid out compactly (Geo::uoff)
  bool compact_ok = false;   // ... which a ragged batch of this many rows may be: every kernel of the route knows that geometry
  struct Stage {
    // all four blocks on the row-owning kernels, their attention on the k | v planes (attention_s.hip where the batch fills its
    // rounds, else attention_pl.hip); false: tile kernels and attention.hip (a stage with one layer whose bound is unusable)
    bool rows = false;
    ResRoute res = RES_TILES;
    bool res_fold = false;   // RES_ROWS: res_conv rides in block1's launch
    bool ln_fold = false;    // the first norm1 is written by the resnet's last launch
    bool qkv_fold = false;   // ... and the first q | k | v too (RES_ONE only)
  } stage[EST_NRES];
};

// estimator.hip
// res_one = false: no whole-resnet launch even where it fits (a solve's shared first step keeps the later steps' resnet route)
EstRoute est_route(const Context& c, long M, bool temb_pre, bool compact, int attn_chunk, bool res_one = true);
// jv_flow_estimator_tap: the stage whose buffer an evaluation copies out before it returns early (null: the whole evaluation)
struct EstTap {
  int id;
  float* out;
  long out_floats;
};
int est_tap_channels(int id);      // channels of a tap's buffer (0: no such tap)
// ahead of an entry's first launch: the tap exists and `out` holds it ([nt, C] for the time taps, [ns, C, T] for the row taps)
int est_tap_check(const EstTap* tap, int ns, int nt, int T);
// the launches up to the stage `tap` names alone (a tap behind TEMB, or none: all four)
int est_tap_time_stages(const EstTap* tap);
// stages: the first so many of the four launches (sinusoid, linear_1, linear_2, the projections)
int time_embedding(Context& c, const float* t, int t_stride, int n, float* sin_buf, float* h1, float* hm, float* emb, hipStream_t st,
                   int stages = 4);
// the estimator body on prepared inputs: ws.xin [rows,320], ws.rowmask/row_sample/lens2, ws.t_dev [B2] -> ws.d [rows,80]
// tap: return behind the launches of that stage, its buffer copied out (the entry has run est_tap_check; XIN is the entry's own)
int estimator_body(Context& c, const Geo& g, const EstRoute& rt, hipStream_t st, const EstTap* tap = nullptr);
#ifdef JV_TUNING
int est_stamps_dump(Context& c, const Geo& g, hipStream_t st);      // JV_RB_STAMPS: print the stamps the last launches left
#endif

}  // namespace jv
