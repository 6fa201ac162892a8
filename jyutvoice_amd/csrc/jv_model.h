// Context, weight registry and per-stage weight views of libjyutvoice_hip.so.
#pragma once
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "jv_common.h"

namespace jv {

// ---- architecture constants (configs/base.yaml:1-110 of the reference; mirrored by spec.py) ------
constexpr int N_FEATS = 80;
constexpr int SPK_DIM = 192;
constexpr int ENC_CH = 192, ENC_HID = 576, ENC_FILTER = 768, ENC_HEADS = 2, ENC_HEAD_DIM = 288, ENC_ROPE = 144,
              ENC_LAYERS = 6;
constexpr int DP_FILTER = 256;
constexpr int EST_IN = 320, EST_CH = 256, EST_TIME = 1024, EST_HEADS = 8, EST_INNER = 512, EST_FF = 1024, EST_NBLK = 4,
              EST_NMID = 12, EST_NRES = 14;
constexpr int NOISE_FRAMES = 15000;
constexpr int HIFT_CH = 512, HIFT_F0_CH = 512, HIFT_NFFT = 16, HIFT_HOP = 4, HIFT_HARM = 9;

constexpr int PR_DIM = 512, PR_HEADS = 8, PR_FFN = 2048, PR_BLOCKS = 6, PR_UP_BLOCKS = 4, PR_VOCAB = 6561;

enum Model : int { MODEL_TTS = 0, MODEL_HIFT = 1, MODEL_PROMPT = 2, MODEL_FLOW = 3 };   // MODEL_FLOW: the decoder.* / spk_embed_affine_layer.* part of MODEL_TTS
// is a tensor of MODEL_TTS part of MODEL_FLOW (what a flow.pt holds besides its encoder)?
inline bool flow_part(const std::string& name) { return name.rfind("decoder.", 0) == 0 || name.rfind("spk_embed_affine_layer.", 0) == 0; }

struct RawTensor {
  std::string name;
  std::vector<int64_t> shape;
  long numel = 0;
  float* dev = nullptr;
  bool loaded = false;
  int model = 0;
};

// simple bump allocator over hipMalloc'd chunks (device memory only; never freed before destroy)
struct Arena {
  std::vector<void*> chunks;
  size_t chunk_floats = (size_t)64 << 20;   // 256 MiB
  size_t used = 0, cap = 0;
  float* cur = nullptr;
  int alloc(size_t floats, float** out);     // 256-byte aligned
  void release();
};

// a packed weight matrix for conv_gemm: rows = output channels, K-contiguous, column j*Cin + ci
struct GemmW {
  const float* w = nullptr;
  const unsigned short* w3 = nullptr;   // three bf16 planes of w (split at load time), plane stride n_rows*ldw
  int ldw = 0, n_rows = 0, N = 0, Cin = 0, ntaps = 1;
  const float* bias = nullptr;
  // fp16x3 path, attached only where a load-time bound on the layer's input exists (registry.hip `half3`):
  const unsigned short* w2 = nullptr;   // two fp16 planes of w[n][:] * 2^e_n
  const unsigned short* wf = nullptr;   // the same two planes in MFMA-fragment order (rowgemm_kernel.h, `Wf`), plane stride N * Cin
  const float* colscale = nullptr;      // 2^-e_n
  float a_scale = 0.f;                  // power of two with bound(|input|) * a_scale < 65504; 0 = no bound, use bf16x6
};

struct LnW { const float* g = nullptr; const float* b = nullptr; };

struct ResnetW {
  GemmW block1, block2, res;
  LnW ln1, ln2;
  // block1's three taps AND res_conv as a fourth fragment step per 32-channel chunk (k-step major fragments: steps 0 .. 3 NCH - 1
  // are block1's, 3 NCH .. 4 NCH - 1 res_conv's), plane stride 256 * 4 * Cin halves: rowconv_wd_kernel<RT, true> (registry.hip)
  const unsigned short* wf4 = nullptr;
  // sqrt(255) max |ln1.g| + max |ln1.b|: the range of block1's LayerNorm, hence (with Mish(v) <= max(v, 0.31) and the time
  // embedding's own maximum) of h2 -- the whole-resnet launch scales its LDS-resident h2 with it (rowres_kernel.h); 0 = n/a
  float h2_bound = 0.f;
  // the weight half of the route (set when the model is finalized, read by est_route):
  bool fold_ok = false;   // block1 has its planes and res_conv can ride in its fragment stream (wf4)
  bool pair_ok = false;   // ... and block2's fragments, every column scale and a usable h2_bound: the whole resnet as one launch
};
struct BtbW {
  LnW n1, n3;
  GemmW qkv, out, ff1, ff2;
  float q_scale = 0.f, k_scale = 0.f, v_scale = 0.f;   // fp16x3 attention (AttnArgs), from the load-time bounds; 0 = bf16x6
  // the weight half of the route (set when the model is finalized, read by est_route and jv_flow_contraction_info):
  int lin_h3 = 0;         // how many of the four linears have fp16 planes and a usable input bound
  bool attn_h3 = false;   // the attention's three scales are usable
  bool rows_ok = false;   // lin_h3 == 4 && attn_h3: the block can run on the row-owning kernels
  bool sk_ok = false;     // to_out and ff.net.2 have split planes at an aligned pitch (split-K tails)
  bool qkv_wf = false;    // q | k | v in fragment order, 256 -> 1536, no bias: a preceding launch can carry it
  bool ffn_wf = false;    // ff.net.0 / ff.net.2 in fragment order, 256 -> 1024 -> 256: the pair as one launch (rowffn_kernel)
  bool block_wf = false;  // ... with to_out (512 -> 256) and the next block's q | k | v too: the fused block (rowblock_kernel.h)
};
struct EstimatorW {
  GemmW time1, time2, temb_all;
  ResnetW res[EST_NRES];                 // 0 = down, 1..12 = mid, 13 = up
  BtbW blk[EST_NRES][EST_NBLK];
  GemmW down_conv, up_conv, final_conv, final_proj;
  LnW final_ln;
  bool stage_rows_ok[EST_NRES] = {};     // all four blocks of the stage: rows_ok
  bool rows_ok = false, sk_ok = false;   // all 56 blocks
  bool mid_pair_ok = false;              // all 12 mid resnets: pair_ok (they ping-pong the trunk together or not at all)
};

struct EncLayerW { GemmW qkv, o, ffn1, ffn2; LnW n1, n2; };
struct EncoderW {
  const float *emb = nullptr, *lang_emb = nullptr, *tone_emb = nullptr, *wpos_emb = nullptr, *spos_emb = nullptr;
  GemmW pre_conv[3], pre_proj;
  LnW pre_ln[3];
  EncLayerW layer[ENC_LAYERS];
  GemmW proj;
  GemmW dp_cond, dp_conv1, dp_conv2, dp_proj;
  LnW dp_ln1, dp_ln2;
  GemmW spk_affine;
};

struct ResBlockW {
  GemmW c1[3], c2[3];
  const float* a1[3];
  const float* a2[3];
  float e1[3] = {}, e2[3] = {};   // max_c 1 / (alpha_c + 1e-9): what Snake can add to |x| (fp16x3 with a measured bound); 0 = n/a
  // the pair in one launch (hiftpair_kernel.h): both convolutions' fragments as one stream (c1's steps, then c2's; plane stride
  // C * 2 k C halves), and the load-time half of the intermediate's bound: c1's largest row L1 norm and largest |bias|
  const unsigned short* wfp[3] = {};
  float l1max[3] = {}, b1max[3] = {};
  int k = 0;
};
struct HiftW {
  GemmW f0_conv[5];
  const float *f0_cls_w = nullptr, *f0_cls_b = nullptr;
  const float *src_lin_w = nullptr, *src_lin_b = nullptr;
  GemmW conv_pre, ups[3], src_down[3], conv_post;
  ResBlockW src_rb[3], rb[9];
};

// prompt branch: FlowEncoder of infer.py:35-83 (Embedding -> UpsampleConformerEncoder -> Linear)
struct ConfBlockW { LnW n_mha, n_ff; GemmW qkv, pos, out, w1, w2; const float *u = nullptr, *v = nullptr; };
struct PromptW {
  const float* emb = nullptr;          // [6561][512]
  const float* div = nullptr;          // [256] positional frequencies (host-computed, embedding.py:239-242)
  GemmW emb_lin, up_emb_lin;           // LinearNoSubsampling.out.0
  LnW emb_ln, up_emb_ln;               // .out.1 with gain and offset pre-multiplied by sqrt(512) (the xscale of the pos-enc)
  GemmW look1, look2, up_conv, proj;
  LnW after;
  ConfBlockW blk[PR_BLOCKS], up[PR_UP_BLOCKS];
};

struct Buf {             // a device allocation owned by the context
  float* p = nullptr;
  size_t floats = 0;
};

struct Context {
  int device = 0;
  int max_batch = 0, max_frames = 0, max_tokens = 0;
  std::vector<RawTensor> raw;
  std::unordered_map<std::string, int> index;
  Arena raw_arena, packed;
  bool ready[4] = {false, false, false, false};
  bool broken = false;           // jv_reserve failed and could not restore the old workspace: every entry point returns JV_ERR_STATE
  EstimatorW est;
  EncoderW enc;
  HiftW hift;
  PromptW prompt;
  float* noise = nullptr;        // [80][15000] fixed CFM noise (device), supplied by the host
  bool noise_loaded = false;
  bool dma_a = false;            // JV_DMA_A=1: fp16x3 linears take their A operand pre-split from the producer (measured slower
                                 // in the pipeline than the in-kernel split; kept as a tested alternative)
  bool no_ffn_fuse = false;      // JV_NO_FFN_FUSE=1: ff.net.0 and ff.net.2 as two launches (the path rowffn_kernel is checked against)
  bool no_temb_pre = false;      // JV_NO_TEMB_PRE=1: the timestep embedding inside every Euler step instead of once per solve (flow.hip cfm_solve)
  bool no_cfg_share = false;     // JV_NO_CFG_SHARE=1: the first Euler step of an equal-length batch on all 2B samples instead of B + 1 (one shared unconditional twin; flow.hip solve_loop)
  bool no_twin_drop = false;     // JV_NO_TWIN_DROP=1: an Euler step whose guidance rate is 0 keeps its unconditional twins (2B samples, CFG update with rate 0) instead of running on B samples (flow.hip solve_loop)
  bool no_ln_fold = false;       // JV_NO_LN_FOLD=1: a stage's first norm1 as its own launch (layernorm256_planes) instead of in the resnet's last convolution
  bool no_res_qkv = false;       // JV_NO_RES_QKV=1: a stage's first q | k | v as its own launch (rowgemm_wa) instead of inside the resnet's (rowres_kernel.h)
  bool no_res_pair = false;      // JV_NO_RES_PAIR=1: a resnet as two row-owning launches (block1 + res_conv, block2) instead of one (rowres_kernel.h)
  bool no_res_fold = false;      // JV_NO_RES_FOLD=1: a resnet's 1 x 1 res_conv as a tile-kernel launch of its own instead of inside block1's row-owning launch
  bool no_compact = false;       // JV_NO_COMPACT=1: ragged batches keep the uniform row geometry (every utterance padded to the longest; flow.hip cfm_solve)
  bool no_qkv_split = false;     // JV_NO_QKV_SPLIT=1: q|k|v stays inside the fused block launch at every batch size (estimator.hip `qkv_split`)
  bool no_block_fuse = false;    // JV_NO_BLOCK_FUSE=1: to_out / feed-forward / next q|k|v as three launches (the path rowblock_kernel is checked against)
  bool no_hift_pair = false;     // JV_NO_HIFT_PAIR=1: a ResBlock's two convolutions as two hiftconv launches (the path hiftpair_kernel is checked against)
  bool no_hiftconv = false;      // JV_NO_HIFTCONV=1: the vocoder's ResBlock convolutions on the tile kernels (A/B aid; the path hiftconv_kernel is checked against)
  bool no_rowgemm = false;       // JV_NO_ROWGEMM=1: keep the transformer linears on the tile kernels at every batch size (A/B aid)
  bool exact_range = false;      // true: bf16x6 everywhere (jv_flow_set_contraction); false: fp16x3 where the range is proven
  bool est_fp16 = false;         // jv_flow_set_precision(JV_PRECISION_FP16) / JV_EST_FP16=1: the estimator's fp16x3 contractions issue the hi x hi product alone (EstRoute::np)
  bool step_graphs = false;      // replay the Euler step as a captured hipGraph (jv_flow_set_graph; never under the profiler)
  std::vector<float> guidance;   // jv_flow_set_guidance: empty = rate 0.7 in every Euler step; one entry = that rate in every step; more = one per step (a solve's n_timesteps must match)
  int solver = 0;                // jv_flow_set_solver: JV_SOLVER_EULER (one estimator evaluation per step) / _MIDPOINT / _HEUN (two; flow.hip solve_loop)
  int enc_attn = 0;              // jv_encoder_set_attention: JV_ENC_ATTN_AUTO / _FUSED / _GEMM (encoder.hip enc_attention_route)
  int attn_chunk = 0;            // > 0: streaming (chunk-causal) estimator attention, in frames (jv_flow_set_streaming)
  // workspace
  std::vector<void*> ws_allocs;
  struct FlowWs* flow = nullptr;
  struct HiftWs* hws = nullptr;
  struct EncWs* ews = nullptr;
  struct PromptWs* pws = nullptr;
  struct AudioWs* aws = nullptr;
  struct ResampleWs* rws = nullptr;   // resampling tables per reduced rate pair (resample.hip): not workspace, survives jv_reserve
  struct FeatWs* fws = nullptr;       // windows, DFT bases, mel weights and per-tile partials of the 16 kHz features (feat16k.hip): not workspace, survives jv_reserve
  struct LevelWs* lws = nullptr;      // K-weighting power tables per sample rate and the per-call intermediates of trim / loudness (level.hip): not workspace, survives jv_reserve
  struct AlignWs* alws = nullptr;     // transposed log prior, decision bits and loss partials of forward() (align.hip): not workspace, survives jv_reserve
  std::string last_error;
};

// a guidance rate (jv_flow_set_guidance, jv_cfm_pool_step_g): finite and >= 0
inline bool guidance_rate_ok(float r) { return std::isfinite(r) && r >= 0.f; }

// registry.hip
void build_registry(Context& c);
int finalize_model(Context& c, int model, hipStream_t st);

// workspace helpers (api.hip)
int ws_alloc(Context& c, size_t bytes, void** out);

// flow.hip
int flow_ws_create(Context& c);
void flow_ws_forget_attention(Context& c, hipStream_t st);   // zero the attention buffer (new weights / contraction mode)
bool flow_has_graphs(const Context& c);
void flow_graphs_drop(Context& c);   // forget captured Euler-step graphs (weights or workspace pointers changed)
struct EstTap;      // flow_ws.h
int flow_estimator(Context& c, const float* x, const int* lens_dev, const float* mu, const float* t_dev, const float* spks,
                   const float* cond, int B2, int T, float* out, hipStream_t st, const float* mask_f32 = nullptr,
                   const EstTap* tap = nullptr);
int flow_estimator_tap(Context& c, int mode, const float* x, const int* lens_dev, const float* mu, const float* t_dev,
                       const float* spks, const float* cond, int B, int T, int tap_id, float* out, long out_floats, hipStream_t st);
int cfm_solve(Context& c, const float* mu, const int* lens_dev, const float* spks, const float* cond, int B, int T,
              int n_timesteps, float temperature, const float* t_span_host, float* mel, hipStream_t st);
int cfm_solve_prompted(Context& c, const float* mu_y, const int* y_lens, const float* prompt_h, const float* prompt_feat,
                       const int* prompt_lens, const float* spks, int B, int Ty, int Ph, int Pf, int n_timesteps,
                       float temperature, const float* t_span_host, float* mel, hipStream_t st);
// in-flight batching (jv_cfm_pool_*): requests in caller-owned pools join and leave a running solve between Euler steps
int cfm_pool_admit(Context& c, const float* mu_y, const float* prompt_h, const float* prompt_feat, const float* spks,
                   const int* h_ylens, const int* h_plens, const int* h_slots, const float* h_temps, int B, int Ty, int Ph, int Pf,
                   float* pool_x, float* pool_mu, float* pool_cond, float* pool_spks, float* pool_amax, int slots, int Tcap,
                   hipStream_t st);
int cfm_pool_step(Context& c, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks, float* pool_amax,
                  int slots, int Tcap, const int* h_slots, const int* h_lens, const float* h_t, const float* h_dt, int B,
                  hipStream_t st, const float* h_cfg = nullptr,      // h_cfg: the guidance rate of every request in this step (null: 0.7)
                  // h_stage (jv_cfm_pool_step_s): the stage of every request's own solver in this step (STAGE_*, jv_ops.h), of which
                  // h_dt is then the coefficient; pool_x0 / pool_k1: the pools the stages save to and read from
                  const int* h_stage = nullptr, float* pool_x0 = nullptr, float* pool_k1 = nullptr);
int cfm_pool_fetch(Context& c, const float* pool_x, int slots, int Tcap, const int* h_slots, const int* h_first, const int* h_lens,
                   int B, int Tm, float* mel, hipStream_t st);

int flow_token2mel(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, const float* prompt_feat,
                   const int* feat_lens, const float* embedding, int B, int P, int N, int F, int streaming, int n_timesteps,
                   float temperature, const float* t_span_host, float* mel, int* mel_lens, hipStream_t st, int ctx = 0,
                   const int* ctx_lens = nullptr);

// encoder.hip: Linear(192 -> 80)(F.normalize(spk)) (jyutvoice_tts.py:175-176, flow.py:315-316)
int speaker_projection(Context& c, const float* spk, int B, float* spks_out, hipStream_t st);
// the four-launch attention of a text-encoder layer on explicit buffers (encoder.hip): scores [B,2,Tt,ld], vt [B,2,288,ld],
// ld = round_up(Tt, 32) <= 512; att rows are written for all Tt rows of every utterance
constexpr int ENC_ATTN_GEMM_MAX = 512;
int enc_attention_gemm(const float* qkv, float* scores, float* vt, float* att, const long* xlen, int B, int Tt, int G, int S,
                       hipStream_t st);
// encattn.hip: the same attention in one launch (online softmax, no [Tt, Tt] buffer); rows L_b <= i < Tt are written as zeros
int enc_attention(const float* qkv, const long* len, int B, int T, int G, int S, float* att, hipStream_t st);

// prompt.hip
int prompt_encoder_fwd(Context& c, const long* tok, const long* len, int B, int Tk, float* h_out, hipStream_t st);
int flow_encoder_fwd(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, int B, int P, int N,
                     int streaming, float* h_out, int* h_lens, hipStream_t st, int ctx = 0);
// per-utterance contexts (jv_flow_encoder_fwd_ctx / jv_flow_token2mel_ctx): the host-side check of the length vectors, then the encoder
int flow_ctx_lengths(const char* who, const long* plen, const long* len, const int* ctx_lens, const int* extra, int B, int P, int N,
                     std::vector<int>& enc_lens, std::vector<int>* extra_host, hipStream_t st);
int flow_encoder_fwd_ctx(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, const int* ctx_lens, int B,
                         int P, int N, int streaming, float* h_out, int* h_lens, hipStream_t st, bool checked);
// the three-GEMM relative-position attention of a conformer block on explicit buffers (prompt.hip); chunk as rel_attention
int rel_attention_gemm(const float* qkv, const float* p, const float* u, const float* v, float* qu, float* qv, float* ac, float* bd,
                       float* vt, float* att, const long* len, int len_mul, int B, int T, int G, int S, int chunk, hipStream_t st);
// relattn.hip: the same attention in one launch (online softmax, no [T, T] buffer); p_rows = rows of p that may be read
int rel_attention(const float* qkv, const float* p, long p_rows, const float* u, const float* v, const long* len, int len_mul, int B,
                  int T, int G, int S, int chunk, float* att, hipStream_t st);
void prompt_ws_destroy(Context& c);

// audio.hip
void audio_ws_destroy(Context& c);

// resample.hip
void resample_ws_destroy(Context& c);

// feat16k.hip
void feat16k_ws_destroy(Context& c);

// align.hip
void align_ws_destroy(Context& c);

// level.hip
void level_ws_destroy(Context& c);

}  // namespace jv

// the opaque handle of include/jyutvoice_hip.h
struct jv_context {
  jv::Context c;
};
