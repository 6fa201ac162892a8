/* libjyutvoice_hip.so -- C ABI of the MI355X-native JyutVoice synthesis hot path.
 *
 * Plain C: opaque context, raw pointers, explicit shapes, a HIP stream passed as void*.  No torch
 * types, no exceptions across the boundary: every call returns JV_OK (0) or an error code and
 * jv_last_error() returns the message.  All work is enqueued on the caller's stream; device
 * pointers are caller-owned unless stated.  The library owns only its context: packed weights and a
 * workspace sized at jv_create().
 *
 * Each entry point names the reference interface it stands in for (paths relative to the
 * indiejoseph/JyutVoice tree).  The precedent for a raw-pointer estimator seam in the reference is the
 * TensorRT path of ConditionalCFM.forward_estimator (jyutvoice/flow/flow_matching.py:267-297), which
 * hands data_ptr()s of x/mask/mu/t/spks/cond to an engine and reads the result from x.
 *
 * Tensor layouts at this boundary are the reference's own: channels-first fp32, e.g. mel [B,80,T].
 */
#ifndef JYUTVOICE_HIP_H
#define JYUTVOICE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JV_OK 0
#define JV_ERR_ARG 1    /* bad argument                                   */
#define JV_ERR_STATE 2  /* weights missing / not finalized                */
#define JV_ERR_HIP 3    /* a HIP runtime call failed                      */
#define JV_ERR_SHAPE 4  /* shape mismatch or capacity exceeded            */
#define JV_ERR_NAME 5   /* unknown tensor name                            */

#define JV_MODEL_TTS 0  /* JyutVoiceTTS state-dict: encoder.*, dp.*, decoder.estimator.*, spk_embed_affine_layer.* */
#define JV_MODEL_HIFT 1 /* HiFTGenerator state-dict                                                                */
#define JV_MODEL_PROMPT 2 /* FlowEncoder state-dict (infer.py:35-83: input_embedding.*, encoder.*, encoder_proj.*) plus the
                             host-computed "pos_enc.div_term" [256] (jyutvoice/transformer/embedding.py:239-242)     */
#define JV_MODEL_FLOW 3 /* the flow decoder alone: the `decoder.*` and `spk_embed_affine_layer.*` tensors of JV_MODEL_TTS -- what a
                           CosyVoice2 flow.pt holds besides its encoder.  Not a registry of its own (jv_tensor_model never returns
                           it): only an argument of jv_finalize                                                     */

typedef struct jv_context jv_context;

/* ---- lifetime -------------------------------------------------------------------------------------
 * Replaces the object graph configs/base.yaml:26-110 builds (JyutVoiceTTS + HiFTGenerator).  Capacity:
 * at most max_batch utterances of max_frames mel frames / max_tokens text tokens per call. */
int jv_create(jv_context** out, int device, int max_batch, int max_frames, int max_tokens);
void jv_destroy(jv_context* ctx);
/* jv_reserve: change the capacities of a live context.  Only the workspace (activation buffers, masks, captured step
 * graphs) is re-created; loaded and finalized weights, the noise tensor and the mel filterbank stay where they are --
 * nothing is uploaded or packed again.  Waits for the device to drain first (it frees buffers queued work may use), so
 * pre-size once with the largest (batch, frames, tokens) a service expects rather than growing call by call.  The
 * reference has no counterpart: its nn.Modules allocate activations per call (infer.py:419-433). */
int jv_reserve(jv_context* ctx, int max_batch, int max_frames, int max_tokens);
/* jv_reserve is failure-atomic: when the new workspace does not fit, the previous capacities are restored and the error is
 * returned; only if that fails as well is the context marked unusable -- jv_usable() then returns 0 and every other entry
 * point JV_ERR_STATE until jv_destroy.  (1 otherwise; 0 for a null context.) */
int jv_usable(const jv_context* ctx);
/* message of the last failing call on this thread (valid until the next failure) */
const char* jv_last_error(void);

/* ---- weights ---------------------------------------------------------------------------------------
 * Replaces tts.load_state_dict(ckpt["state_dict"]) / hift.load_state_dict(torch.load(hift.pt))
 * (infer.py:343-351).  Names and shapes are the checkpoint's own keys; the registry is enumerable so
 * a loader can validate a checkpoint before touching the GPU. */
int jv_num_tensors(const jv_context* ctx);
const char* jv_tensor_name(const jv_context* ctx, int i);
int jv_tensor_model(const jv_context* ctx, int i);
int jv_tensor_ndim(const jv_context* ctx, int i);
int64_t jv_tensor_dim(const jv_context* ctx, int i, int d);
/* copy one fp32 tensor (host or device memory) into the context */
int jv_load_tensor(jv_context* ctx, const char* name, const float* data, const int64_t* shape, int ndim, int on_device,
                   void* stream);
/* the CFM's fixed noise tensor [1,80,15000] (CausalConditionalCFM.rand_noise, flow_matching.py:353-354: a plain
 * attribute, not a state-dict entry; the host regenerates it from torch seed 0) */
int jv_load_noise(jv_context* ctx, const float* data, int64_t numel, int on_device, void* stream);
/* all tensors of `model` present -> fold weight-norm, pack GEMM operands.  Errors name the missing key.
 * JV_MODEL_FLOW asks only for the `decoder.*` and `spk_embed_affine_layer.*` tensors of JV_MODEL_TTS (same slots, same packing)
 * and makes the estimator, the solver and the speaker projection usable: jv_flow_estimator_*, jv_cfm_solve*, jv_flow_token2mel.
 * JV_MODEL_TTS keeps asking for all of its tensors and implies JV_MODEL_FLOW; after JV_MODEL_FLOW it packs the rest.  The text-side
 * entries (jv_encoder_fwd) on a flow-only context return JV_ERR_STATE naming what is missing. */
int jv_finalize(jv_context* ctx, int model, void* stream);

/* ---- flow decoder ------------------------------------------------------------------------------------
 * jv_flow_estimator_step: CausalConditionalDecoder.forward (jyutvoice/flow/decoder.py:917-1018) through the
 * forward_estimator seam (flow_matching.py:267-297).  x, mu, cond, out: [B2,80,T]; t: [B2]; spks: [B2,80];
 * lens: [B2] int32 valid frames per row (NULL = all T), the key-padding mask of decoder.py:951-959 (see "Lengths" below).
 * out may alias x (the TRT seam writes its result into x).
 *
 * Lengths.  Every lens[b] passed to jv_flow_estimator_step, jv_cfm_solve, jv_hift_f0 and jv_hift_decode MEANS
 * min(max(lens[b], 0), T) -- the reference's sequence_mask(lens, T): an entry above T is the full length, a negative one is 0,
 * in the uniform row geometry and in the compact one of ragged batches alike (the result is the same bits as the call with the
 * clamped value).  An utterance of effective length 0 comes back as zeros and changes nothing in the other utterances; none of
 * its inputs is read.  Output frames / samples behind an utterance's length are zeros.  jv_cfm_solve_prompted and
 * jv_mel_spectrogram_ragged do not clamp: they REJECT a length outside their stated range (JV_ERR_ARG naming the utterance). */
int jv_flow_estimator_step(jv_context* ctx, const float* x, const int32_t* lens, const float* mu, const float* t,
                           const float* spks, const float* cond, int B2, int T, float* out, void* stream);
/* jv_flow_estimator_masked: the same call with the six named tensors of the TensorRT seam exactly as
 * ConditionalCFM.forward_estimator binds them (flow_matching.py:270-290; profile shapes scripts/export_onnx.py:343-346):
 * mask is the reference's own float mask [B2,1,T] (1 = frame, 0 = padding) instead of lengths; the result may be written
 * into x (the seam passes x.data_ptr() as the output address).  jyutvoice_amd.flow.estimator.HipEstimator wraps it. */
int jv_flow_estimator_masked(jv_context* ctx, const float* x, const float* mask, const float* mu, const float* t,
                             const float* spks, const float* cond, int B2, int T, float* out, void* stream);
/* jv_flow_estimator_tap (used by the parity tests): the launch sequence of ONE estimator evaluation up to and including one stage,
 * whose buffer is copied out channels-first.  It runs the function the production entries run (Est::run, estimator.hip) with a
 * tap descriptor: the same argument checks, row layout and route decision, the same launches in the same order; the launches
 * behind the tap are not run, and an untapped call launches what it launched without this entry.  Two modes:
 *   JV_EST_MODE_ENTRY  jv_flow_estimator_step: B = B2 samples as the caller gives them, t [B] one timestep per sample, uniform rows,
 *                      the time embedding made inside the evaluation.  x, mu, cond [B,80,T], spks [B,80], lens [B] or NULL.
 *   JV_EST_MODE_STEP   one evaluation of a step of jv_cfm_solve: B utterances laid out with their B unconditional twins (2B
 *                      samples: twin b at sample B + b carries x of utterance b and zeros for mu, spks, cond), t [1] one timestep
 *                      for all, its embedding made ahead of the evaluation as the solve makes every step's, the compact geometry of
 *                      ragged batches exactly where jv_cfm_solve takes it (its one synchronisation included).  x, mu, cond
 *                      [B,80,T], spks [B,80], lens [B] or NULL.  The only way to the whole-resnet launch and the compact tables.
 *                      It is a step of the DEFAULT solve: always 2B samples and the embedding always made ahead.  A solve whose
 *                      guidance rates are all 0 lays out B samples, and one under JV_NO_TEMB_PRE=1 or with more than 64 evaluations
 *                      makes the embedding inside every evaluation; neither form is reachable here (the latter is ENTRY's).
 * The context modes (jv_flow_set_streaming, _contraction, _precision) apply as to the entry mirrored.  Another mode or an unknown
 * tap: JV_ERR_ARG; out_floats too small for the tap: JV_ERR_SHAPE; both behind the entry's own checks and ahead of its first launch.
 * With S = B (ENTRY) or 2B (STEP) samples and n = B (ENTRY) or 1 (STEP) timesteps, taps in execution order (79 ids, 0 .. 78):
 *   TSIN [n,320]  sin | cos of 1000 t f_j      T1 [n,1024]  SiLU(linear_1)      TMISH [n,1024]  Mish(linear_2)
 *   TEMB [n,14 x 256]  the 14 resnets' projections of it, stage i at columns 256 i
 *   XIN [S,320,T]  x | mu | spks | cond
 *   RESi [S,256,T]  the resnet of stage i = 0 .. 13 (0: down, 1 .. 12: mid, 13: up, which reads cat[BLK12_3, BLK0_3])
 *   BLKi_j [S,256,T]  transformer block j = 0 .. 3 of stage i (BLK0_3 is the skip connection)
 *   DOWN, UPC [S,256,T]  the causal convolutions behind stage 0 and stage 13;  FIN [S,256,T]  final conv + LayerNorm + Mish + mask
 *   D [S,80,T]  the projection: the entry's output
 * Row taps hold exact zeros at and behind every sample's clamped length.  Stage 0 owns ids JV_EST_TAP_RES0 .. + 4 (its resnet and
 * four blocks), stage i >= 1 ids JV_EST_TAP_RES1 + JV_EST_TAP_PER_STAGE (i - 1) .. + 4. */
#define JV_EST_MODE_ENTRY 0
#define JV_EST_MODE_STEP 1
#define JV_EST_TAP_TSIN 0
#define JV_EST_TAP_T1 1
#define JV_EST_TAP_TMISH 2
#define JV_EST_TAP_TEMB 3
#define JV_EST_TAP_XIN 4
#define JV_EST_TAP_RES0 5      /* BLK0_j = 6 + j */
#define JV_EST_TAP_DOWN 10
#define JV_EST_TAP_RES1 11     /* stage i >= 1: RESi = 11 + JV_EST_TAP_PER_STAGE (i - 1), BLKi_j = RESi + 1 + j */
#define JV_EST_TAP_PER_STAGE 5
#define JV_EST_TAP_UPC 76
#define JV_EST_TAP_FIN 77
#define JV_EST_TAP_D 78
#define JV_EST_TAP_COUNT 79
int jv_flow_estimator_tap(jv_context* ctx, int mode, const float* x, const int32_t* lens, const float* mu, const float* t,
                          const float* spks, const float* cond, int B, int T, int tap, float* out, int64_t out_floats, void* stream);
/* jv_flow_set_streaming: the `streaming=True` mode of CausalConditionalDecoder.forward (decoder.py:951-954, 976-979,
 * 999-1002 -> utils/mask.py:91-126,192-198): chunk-causal attention with static_chunk_size = chunk_frames (50 in
 * configs/base.yaml:98) and all left chunks; 0 restores full attention.  Applies to the following estimator / solver
 * calls on this context. */
int jv_flow_set_streaming(jv_context* ctx, int chunk_frames);
/* jv_flow_set_graph: jv_cfm_solve replays one Euler step (step scalars -> estimator input -> estimator -> CFG update,
 * flow_matching.py:230-265) as a captured hipGraph per (B, T, attention mode), on a private stream fenced against
 * `stream` with events; the step reads (t, dt) through a device-side counter so one graph serves every step.  Off by
 * default (on = 1 here, or JV_STEP_GRAPH=1 in the environment at jv_create, turns it on): on MI355X / ROCm 7.2 the replay
 * measured 0.4 % (B = 32, T = 300) to 5 % (B = 1, T = 128) slower than the eager launches, which already run ahead of
 * the GPU.  The in-library profiler (jv_profile_enable) forces the eager path because it brackets every
 * launch with events.  Results are bit-identical either way. */
int jv_flow_set_graph(jv_context* ctx, int on);
/* jv_flow_set_guidance: the classifier-free-guidance rate of ConditionalCFM.solve_euler (flow_matching.py:215-265,
 * `inference_cfg_rate` of configs/base.yaml: x += dt ((1 + r) v(x, t | mu, spks, cond) - r v(x, t))), a context mode like
 * jv_flow_set_streaming.  rates_host: n host floats, read before the call returns.  n = 0 (or rates_host = NULL): the default,
 * 0.7 in every step.  n = 1: that rate in every step.  n > 1: one rate per Euler step -- a guidance window is the usual form --
 * and a solve whose n_timesteps != n fails with JV_ERR_ARG naming both numbers before its first launch.  A rate must be finite
 * and >= 0, else JV_ERR_ARG (the mode is then unchanged).  Read by every closed solve: jv_cfm_solve, jv_cfm_solve_prompted,
 * jv_flow_token2mel, _partial and _ctx; not by jv_flow_estimator_step / _masked, which have no solver, nor by jv_cfm_pool_step
 * (jv_cfm_pool_step_g takes a rate per request).  The rate reaches the update through a device table stepped with the step
 * counter, as dt does, so a captured step (jv_flow_set_graph) replays with the rate of ITS step.
 * NO-TWIN STEPS.  A step whose rate is exactly 0 needs no unconditional evaluation and runs on B samples, x += dt v(x, t | ...):
 * a solve whose rates are all 0 never lays out, packs or computes a twin; a solve with mixed rates changes between the 2B- and
 * the B-sample rows from step to step where both take the same estimator route (both beyond the 2048-row split-K seam, the same
 * resnet launches, uniform rows) and otherwise keeps the twins in that step, where the update with rate 0 gives the same x.
 * Either way the result meets the twin-keeping one within the bound of any change of batch geometry (2e-5).  Such solves are
 * always eager.  JV_NO_TWIN_DROP=1 in the environment at jv_create keeps the twins in every step (for A/B runs).  With the
 * default and with 0.7 set explicitly the update is the same fp32 operations in the same order as before this mode existed. */
int jv_flow_set_guidance(jv_context* ctx, const float* rates_host, int n);
/* jv_flow_set_solver: the integrator of the closed solves, a context mode like jv_flow_set_guidance, read by the same entries
 * (jv_cfm_solve, jv_cfm_solve_prompted, jv_flow_token2mel, _partial and _ctx).  With (t_k, dt_k) of step k exactly as before (the
 * fp32 running recurrence over t_span) and g(x, t) = (1 + r_k) v(x, t | mu, spks, cond) - r_k v(x, t), in fp32 in this order:
 *   JV_SOLVER_EULER (default): x <- x + dt g(x, t) -- ConditionalCFM.solve_euler (flow_matching.py:215-265), unchanged: the same
 *     launches and the same bits as before this mode existed.
 *   JV_SOLVER_MIDPOINT: xs = x + (0.5f dt) g(x, t);  x <- x + dt g(xs, t + 0.5f dt).
 *   JV_SOLVER_HEUN:     k1 = g(x, t);  xs = x + dt k1;  x <- x + (0.5f dt) (k1 + g(xs, t + dt)).
 * n_timesteps stays the number of STEPS: a second-order solve performs 2 n_timesteps estimator evaluations, and one whose
 * evaluations exceed 1024 fails with JV_ERR_ARG naming both numbers before its first launch.  The guidance rate of step k (and
 * so the step without twins behind a rate of exactly 0) holds for both of its evaluations; a guidance schedule still holds one rate
 * per step.  Second-order solves always run eagerly on 2B (or B) samples: the captured graph of jv_flow_set_graph is an Euler step
 * and replays for Euler solves only, and the shared twin of the first Euler step is not taken.  An unknown value fails with
 * JV_ERR_ARG and leaves the mode unchanged.  Not read by jv_cfm_pool_step / _g (Euler); jv_cfm_pool_step_s takes a stage per request. */
#define JV_SOLVER_EULER 0
#define JV_SOLVER_MIDPOINT 1
#define JV_SOLVER_HEUN 2
int jv_flow_set_solver(jv_context* ctx, int solver);
/* jv_flow_set_contraction: how fp32 contractions are carried out on the 16-bit matrix cores.  exact_range = 0
 * (default): fp16x3 -- each operand split into two fp16 planes after an exact power-of-two scaling (22 significant bits,
 * three MFMA products, fp32 accumulate) -- wherever an upper bound of the operand is known, so that fp16's range cannot be
 * exceeded: PROVEN from the weights at load time for the estimator's Linear layers and attention (transformer.py:355-443:
 * LayerNorm outputs, Linears of bounded inputs, attention outputs, GELU of a bounded Linear), MEASURED on the device by the
 * kernels that produce the operand for the estimator's convolutions (decoder.py:110-115, 767-788) and the vocoder
 * (generator.py:90-97, 396-432).  Every other contraction, and all of them with exact_range = 1 (or JV_EXACT_RANGE=1 in
 * the environment at jv_create), runs bf16x6 (three bf16 planes, 24 bits, six products), which takes any fp32 operand.
 * Both meet the same operator-level bound against fp64 (tests/test_gpu_ops.py).  Applies to this context's estimator,
 * solver and vocoder calls. */
int jv_flow_set_contraction(jv_context* ctx, int exact_range);
/* jv_flow_set_precision: the estimator as the reference's fp16 TensorRT plan runs it (scripts/export_onnx.py:342-361,
 * `fp16 = True`; flow_matching.py:267-297).  JV_PRECISION_FP32 (default): every contraction at fp32 accuracy, as
 * jv_flow_set_contraction describes.  JV_PRECISION_FP16 (or JV_EST_FP16=1 in the environment at jv_create): in an estimator
 * evaluation (jv_flow_estimator_step / _masked, every jv_cfm_solve* and jv_flow_token2mel*) each contraction that the route
 * would run fp16x3 issues the hi x hi product alone -- operands rounded to fp16 (11 significant bits) under the same
 * power-of-two scales, products exact in fp32, fp32 accumulation.  Nothing else changes: scales, bounds, the planes producers
 * write (both; the lo plane is not multiplied), the fp32 residual stream, epilogues, LayerNorm, softmax, routes, regimes and
 * launch geometry; the contractions that run bf16x6 (the first resnet's input convolutions, the time MLP, any layer whose
 * bound is unusable: jv_flow_contraction_info); the encoders, the prompt path and the vocoder.  The invariances of the fp32
 * mode (batch row = its B = 1 run, compact = padded, streamed prefix = one-shot) hold inside the mode with the same bounds.
 * A configuration call like jv_flow_set_contraction: it waits for the device and drops captured step graphs.  FP16 together
 * with exact_range = 1 is a contradiction (bf16x6 has nothing to drop): whichever of the two setters comes second returns
 * JV_ERR_STATE. */
#define JV_PRECISION_FP32 0
#define JV_PRECISION_FP16 1
int jv_flow_set_precision(jv_context* ctx, int precision);
/* jv_flow_contraction_info: what the load-time range proofs of the last jv_finalize(JV_MODEL_TTS) concluded for the
 * estimator's 56 transformer blocks (transformer.py:355-443; registry.hip), so that a caller -- or a test with a hostile
 * checkpoint -- can see which layers took the fp16x3 engine and which stayed on bf16x6 because their bound was unusable
 * (non-finite or beyond 1e30).  out[0] = blocks, out[1] = blocks whose four linears AND attention all have a usable bound,
 * out[2] = linears (of 4 per block) with a usable bound, out[3] = blocks whose attention operands (q, k, v) have one.
 * n = number of int32 slots in out (>= 4); with n >= 5, out[4] = the precision mode (jv_flow_set_precision), which changes none
 * of the other four. */
int jv_flow_contraction_info(const jv_context* ctx, int32_t* out, int n);
/* jv_cfm_solve: CausalConditionalCFM.forward + ConditionalCFM.solve_euler (flow_matching.py:356-401, 215-265):
 * fixed noise prefix * temperature, cosine schedule, n_timesteps Euler steps with CFG rate 0.7.
 * mu, cond, mel: [B,80,T]; spks: [B,80]; lens: [B] int32 or NULL ("Lengths" above: clamped to [0, T]).  t_span_host: optional n_timesteps+1 host floats
 * (the caller's own 1-cos(linspace*pi/2)); NULL = computed here.  B > 1 is the batched extension, defined as the
 * per-utterance loop of the batch-1-only reference. */
int jv_cfm_solve(jv_context* ctx, const float* mu, const int32_t* lens, const float* spks, const float* cond, int B, int T,
                 int n_timesteps, float temperature, const float* t_span_host, float* mel, void* stream);
/* jv_cfm_solve_prompted: the voice-cloning glue of JyutVoiceTTS.synthesise (jyutvoice_tts.py:213-244: mu = [prompt_h | mu_y],
 * cond = [prompt_feat | 0], the solve over all p + y frames, `decoder_outputs[:, :, mel_len1:]`) around the same solver, for a
 * batch in which EVERY utterance has a prompt of its own length -- defined as the batch-1 reference looped over the utterances,
 * utterance b called with prompt_h[b, :p_b] and prompt_feat[b, :p_b].  Its sequence is p_b + y_b frames, the noise column j
 * belongs to frame j of its own sequence, and mel[b, :, :y_b] receives frames p_b .. p_b + y_b - 1 (zeros behind y_b).
 * mu_y, mel: [B,80,Ty]; y_lens, prompt_lens: [B] int32; prompt_h: [B,Ph,80], prompt_feat: [B,Pf,80] (batch, time, channel;
 * 16-byte aligned; what lies behind p_b is not read); spks: [B,80].  All device pointers except t_span_host (as jv_cfm_solve).
 * 0 <= prompt_lens[b] <= min(Ph, Pf) and 0 <= y_lens[b] <= Ty, else JV_ERR_ARG naming the utterance, before anything is
 * launched (both vectors come down with the solve's one synchronisation); p_b = 0 is the unprompted solve of that utterance.
 * The capacity of jv_create / jv_reserve applies to T = max_b(p_b + y_b). */
int jv_cfm_solve_prompted(jv_context* ctx, const float* mu_y, const int32_t* y_lens, const float* prompt_h,
                          const float* prompt_feat, const int32_t* prompt_lens, const float* spks, int B, int Ty, int Ph, int Pf,
                          int n_timesteps, float temperature, const float* t_span_host, float* mel, void* stream);
/* ---- in-flight batching: requests join and leave a running solve between two Euler steps ---------------------------------
 * The solver's state between two steps of ConditionalCFM.solve_euler (flow_matching.py:230-265) is x, the running trunk maxima
 * that the fp16x3 scales derive from, and a step counter; the estimator takes one t per sample.  So the utterances of one
 * estimator evaluation need not be at the same step.  A request's state lives in caller-owned device pools, moved by descriptor
 * like the pools of jv_slab_copy's callers; the library keeps nothing about a request between calls:
 *   pool_x, pool_mu, pool_cond [slots, Tcap, 80] fp32, frame-major (the layout of prompt_h / prompt_feat), 16-byte aligned;
 *   pool_spks [slots, 80], the projected speaker vector;  pool_amax [slots, 3, 2], the running maxima of the request and of its
 *   CFG twin, one per tracked trunk buffer.
 * A request served this way is DEFINED as jv_cfm_solve_prompted at B = 1 with its own n_timesteps and temperature, whatever else
 * is in the pool and whenever the others joined or left; it meets it within the bound of any change of batch geometry (2e-5).
 * Every per-request scalar is a HOST array (*_host): the caller decides them on the host anyway.  No call synchronises, and none
 * keeps a pointer to a host array after it returns (the values travel as kernel arguments).  Every call validates all of its
 * arguments before its first launch: a rejected call (JV_ERR_ARG / JV_ERR_SHAPE naming the request) leaves the pools unchanged.
 *
 * jv_cfm_pool_admit: packs B new requests into their slots.  mu_y [B,80,Ty], prompt_h [B,Ph,80], prompt_feat [B,Pf,80], spks
 *   [B,80] on the device as for jv_cfm_solve_prompted; y_lens, prompt_lens, slots [B] int32 and temperature [B] float on the host.
 *   Slot s receives mu = [prompt_h[b, :p_b] | mu_y[b, :, :y_b]], cond = [prompt_feat[b, :p_b] | 0], x = noise[:, :p_b + y_b] *
 *   temperature[b], spks[b], and zeroed maxima.  0 <= p_b <= min(Ph, Pf), 0 <= y_b <= Ty, 1 <= p_b + y_b <= Tcap, 0 <= slot <
 *   slots, no slot twice.  Rows of a slot behind p_b + y_b are neither written nor ever read.
 * jv_cfm_pool_step: ONE Euler + CFG step (rate 0.7) for the B listed slots, request b at (t_host[b], dt_host[b]) with lens_host[b]
 *   = p_b + y_b frames: x += dt_b ((1 + 0.7) v(x, t_b | mu, spks, cond) - 0.7 v(x, t_b)).  The rows are laid out by the rule of
 *   jv_cfm_solve (compact where the estimator's route allows it, else uniform, padded to the step's longest request), always
 *   two rows per frame (no shared first-step twin), always eager.  The context modes (jv_flow_set_streaming, _contraction,
 *   _precision) apply as to any estimator call.  1 <= B <= max_batch, 1 <= lens_host[b] <= min(Tcap, max_frames), slots in range,
 *   none twice.
 * jv_cfm_pool_fetch: mel[b, :, t] = pool_x[slots_host[b], first_host[b] + t, :] for t < lens_host[b], zeros behind, mel [B,80,Tm]
 *   -- the unpack of jv_cfm_solve_prompted with first = p_b, len = y_b.  0 <= first_b, 0 <= len_b <= Tm, first_b + len_b <= Tcap.
 * jv_cfm_pool_step_g: jv_cfm_pool_step with cfg_host[B], the guidance rate of each listed request in THIS step (finite and >= 0;
 *   flow_matching.py:215-265 with the request's own inference_cfg_rate, or its guidance window's rate at this t): x += dt_b ((1 +
 *   cfg_b) v(x, t_b | ...) - cfg_b v(x, t_b)).  jv_cfm_pool_step is this call with 0.7 for all, bit for bit.  A pool step always
 *   carries two rows per frame, also for a request at rate 0: its twin is computed and (1 + 0) v_c - 0 v_u is v_c.  Dropping the
 *   twins of individual requests inside a step (a mixed twin map) is a follow-up.
 * jv_cfm_pool_step_s: jv_cfm_pool_step_g for requests with a solver of their own (jv_flow_set_solver's definitions): a request on
 *   a second-order solver takes TWO pool steps per solver step, and every listed request is taken at its own stage_host[b] with
 *   the coefficient coef_host[b], at time t_host[b].  With g = (1 + cfg_b) v(x, t_b | ...) - cfg_b v(x, t_b) and x = pool_x[slot]:
 *     JV_STAGE_EULER  c = dt:      x <- x + c g                                   (jv_cfm_pool_step_g, bit for bit)
 *     JV_STAGE_MID1   c = 0.5f dt: x0 <- x;  x <- x + c g                         (t_b = t)
 *     JV_STAGE_MID2   c = dt:      x <- x0 + c g                                  (t_b = t + 0.5f dt)
 *     JV_STAGE_HEUN1  c = dt:      x0 <- x;  k1 <- g;  x <- x + c g               (t_b = t)
 *     JV_STAGE_HEUN2  c = 0.5f dt: x <- x0 + c (k1 + g)                           (t_b = t + dt)
 *   pool_x0, pool_k1: [slots, Tcap, 80] like pool_x, caller-owned, 16-byte aligned; either may be NULL where no listed stage
 *   touches it (Euler: neither, midpoint: pool_x0 only), else JV_ERR_ARG naming the request.  pool_x always holds the estimator's
 *   next input, so between a step's two stages jv_cfm_pool_fetch would return the stage point: fetch after the last stage.  The
 *   running maxima accumulate over all evaluations.  A request served this way is DEFINED as jv_cfm_solve_prompted at B = 1 under
 *   jv_flow_set_solver with its solver, within the same 2e-5. */
int jv_cfm_pool_admit(jv_context* ctx, const float* mu_y, const float* prompt_h, const float* prompt_feat, const float* spks,
                      const int32_t* y_lens_host, const int32_t* prompt_lens_host, const int32_t* slots_host,
                      const float* temperature_host, int B, int Ty, int Ph, int Pf, float* pool_x, float* pool_mu, float* pool_cond,
                      float* pool_spks, float* pool_amax, int slots, int Tcap, void* stream);
int jv_cfm_pool_step(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                     float* pool_amax, int slots, int Tcap, const int32_t* slots_host, const int32_t* lens_host, const float* t_host,
                     const float* dt_host, int B, void* stream);
int jv_cfm_pool_step_g(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                       float* pool_amax, int slots, int Tcap, const int32_t* slots_host, const int32_t* lens_host, const float* t_host,
                       const float* dt_host, const float* cfg_host, int B, void* stream);
#define JV_STAGE_EULER 0
#define JV_STAGE_MID1 1
#define JV_STAGE_MID2 4
#define JV_STAGE_HEUN1 3
#define JV_STAGE_HEUN2 12
int jv_cfm_pool_step_s(jv_context* ctx, float* pool_x, const float* pool_mu, const float* pool_cond, const float* pool_spks,
                       float* pool_amax, float* pool_x0, float* pool_k1, int slots, int Tcap, const int32_t* slots_host,
                       const int32_t* lens_host, const float* t_host, const float* coef_host, const float* cfg_host,
                       const int32_t* stage_host, int B, void* stream);
int jv_cfm_pool_fetch(jv_context* ctx, const float* pool_x, int slots, int Tcap, const int32_t* slots_host, const int32_t* first_host,
                      const int32_t* lens_host, int B, int Tm, float* mel, void* stream);

/* ---- prompt (voice-cloning) branch ---------------------------------------------------------------------
 * jv_prompt_encoder_fwd: FlowEncoder.forward of the reference's infer.py:35-83 -- Embedding(clamp(token, 0)) * mask ->
 * UpsampleConformerEncoder(streaming=False) (jyutvoice/transformer/upsample_encoder.py:329-375) -> Linear(512, 80): the
 * `prompt_h` that JyutVoiceTTS.synthesise prepends to mu (jyutvoice_tts.py:213-225).
 * tokens: int64 [B,Tk] speech-token ids (< 6561), token_len: int64 [B]; prompt_h: [B, 2*Tk, 80] (batch, time, channel),
 * zero beyond 2*token_len[b].  B > 1 is the per-utterance loop of the B = 1 reference usage.  2*Tk <= max_frames. */
int jv_prompt_encoder_fwd(jv_context* ctx, const int64_t* tokens, const int64_t* token_len, int B, int Tk, float* prompt_h,
                          void* stream);

/* ---- token-to-mel: CausalMaskedDiffWithXvec.inference (jyutvoice/flow/flow.py:300-358), finalize=True ------------------------
 * jv_flow_encoder_fwd: flow.py:319-328, 338 -- utterance b's token sequence is [prompt_tokens[b, :p_b] | tokens[b, :n_b]]
 * (concatenated inside the embedding kernel; what lies behind either length is not read), Embedding(clamp(token, 0)) * mask ->
 * UpsampleConformerEncoder(streaming) -> Linear(512, 80).  prompt_tokens: int64 [B,P] (P = 0: none, the pointers may be NULL),
 * tokens: int64 [B,N]; prompt_lens, token_lens: int64 [B], clamped to [0, P] / [0, N]; h: [B, 2*(P+N), 80] (batch, time, channel),
 * zeros behind 2*(p_b + n_b); h_lens: optional [B] int32, receives 2*(p_b + n_b).  streaming != 0: the chunk masks of
 * upsample_encoder.py:338-367 (static_chunk_size 25 tokens, 50 after the up-sampling, all left chunks; the look-ahead convolution
 * reaches across chunk edges as in the reference).  The relative-position attention is ONE launch per block (relattn.hip, online
 * softmax): this route's workspace holds no [T, T] buffer.  Needs JV_MODEL_PROMPT; 2*(P+N) <= max_frames, P+N <= 2048.
 * jv_flow_token2mel: the rest of flow.py:314-358 for a batch -- F.normalize + spk_embed_affine_layer, mu = h, cond = [prompt_feat_b
 * [:f_b] | 0], the solver of jv_cfm_solve over T_b = 2*(p_b + n_b) frames (with the estimator's streaming mask when streaming != 0,
 * restored afterwards), and frames f_b .. T_b - 1 left-aligned in mel[b] with zeros behind y_b = T_b - f_b.  Noise column j belongs
 * to frame j of the utterance's own sequence.  B > 1 is the B = 1 reference looped over the utterances.
 * prompt_feat: [B,F,80] (batch, time, channel; 16-byte aligned; F = 0: none); feat_lens: [B] int32 f_b; embedding: [B,192] raw;
 * mel: [B,80,Tm], Tm = 2*(P+N); mel_lens: optional [B] int32, receives y_b.  0 <= f_b <= min(F, T_b), else JV_ERR_ARG naming the
 * utterance, before the solve is launched (a wrong f_b is a wrong split point, which a clamp would turn into other frames silently:
 * the rule of jv_cfm_solve_prompted).  Needs JV_MODEL_PROMPT and JV_MODEL_FLOW (or JV_MODEL_TTS) and the noise tensor. */
int jv_flow_encoder_fwd(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                        const int64_t* token_lens, int B, int P, int N, int streaming, float* h, int32_t* h_lens, void* stream);
int jv_flow_token2mel(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                      const int64_t* token_lens, const float* prompt_feat, const int32_t* feat_lens, const float* embedding, int B,
                      int P, int N, int F, int streaming, int n_timesteps, float temperature, const float* t_span_host, float* mel,
                      int32_t* mel_lens, void* stream);
/* Partial sequences, B = 1 -- what flow.py:327-336 (`finalize=False`) intends: of the m = P + N tokens the last
 * pre_lookahead_len = 3 are look-ahead context only (`token[:, -3:]`, flow.py:330-333).  They are embedded row-wise like the
 * others (upsample_encoder.py:446-453, forward_chunk) and read by PreLookaheadLayer.conv1 alone, in place of its zero padding
 * (upsample_encoder.py:110-121); the encoder, every length and mask, the solve and the unpack run on L = m - 3 tokens.  A caller
 * that feeds tokens as they arrive gets, with streaming != 0 and L a multiple of 25, frames that no later token changes.
 * jv_flow_encoder_fwd_partial: h [1, 2 L, 80], h_lens receives 2 (p + n - 3).
 * jv_flow_token2mel_partial: mel [1, 80, 2 L], frames f .. 2 L - 1 left-aligned, mel_lens receives 2 L - f; 0 <= f <= min(F, 2 L).
 * Arguments as in the whole-sequence entries with B = 1; P + N >= 4, else JV_ERR_ARG.  The whole-sequence entries run the same code
 * with a context of 0 tokens: their launches and bits are unchanged. */
int jv_flow_encoder_fwd_partial(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                                const int64_t* token_lens, int P, int N, int streaming, float* h, int32_t* h_lens, void* stream);
int jv_flow_token2mel_partial(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                              const int64_t* token_lens, const float* prompt_feat, const int32_t* feat_lens, const float* embedding,
                              int P, int N, int F, int streaming, int n_timesteps, float temperature, const float* t_span_host,
                              float* mel, int32_t* mel_lens, void* stream);
/* A look-ahead context PER UTTERANCE -- a batch that mixes partial sequences (sessions in mid-stream) with whole ones (sessions
 * that finish): the whole-sequence entries with one more argument, ctx_lens [B] int32 on the device, each entry 0 or 3.  Of
 * utterance b's m_b = p_b + n_b tokens the last ctx_b are look-ahead context only, as above; every length and mask, the solve and
 * the unpack run on L_b = m_b - ctx_b.  The buffers keep the whole-sequence widths: h [B, 2 (P + N), 80], mel [B, 80, 2 (P + N)];
 * h_lens receives 2 L_b, mel_lens 2 L_b - f_b; 0 <= f_b <= min(F, 2 L_b).  B > 1 is the B = 1 entries looped over the utterances
 * (jv_flow_*_partial where ctx_b = 3, the whole-sequence entry where it is 0).  The token counts and ctx_lens come down to the host
 * and are checked before anything is launched on them -- the call's one synchronisation; jv_flow_encoder_fwd_ctx, which has no
 * other, takes one for this: ctx_b outside {0, 3} or m_b - ctx_b < 1 is JV_ERR_ARG naming the utterance.  `streaming` is one flag
 * for the call. */
int jv_flow_encoder_fwd_ctx(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                            const int64_t* token_lens, const int32_t* ctx_lens, int B, int P, int N, int streaming, float* h,
                            int32_t* h_lens, void* stream);
/* jv_upsample_encoder_tap (used by the parity tests): the launch sequence of one of the four entries above up to and including one
 * stage of the UpsampleConformerEncoder, whose workspace buffer is then copied out -- an early return inside the function those
 * entries run (the buffers ping-pong and the hidden state is updated in place, so a stage can only be read where it stands), not
 * a second sequence: the argument checks, the lengths, the row masks and every launch ahead of the return are the entry's own.
 * mode selects the entry: JV_UPS_MODE_PROMPT (jv_prompt_encoder_fwd: P must be 0 and streaming 0, the three-GEMM attention),
 * JV_UPS_MODE_FLOW (jv_flow_encoder_fwd), JV_UPS_MODE_PARTIAL (jv_flow_encoder_fwd_partial: B must be 1) and JV_UPS_MODE_CTX
 * (jv_flow_encoder_fwd_ctx; ctx_lens is read by this mode alone).  Another mode or an unknown tap: JV_ERR_ARG; out_floats too
 * small for the tap: JV_ERR_SHAPE; both behind the entry's own checks and ahead of its first launch.
 * Layout, with W = P + N (the width of the whole sequence in every mode) and L_b the encoded length (p_b + n_b less the context):
 *   row taps   out [B, C, W] (token rate) or [B, C, 2 W] (mel rate), channels first; exact zeros at and behind L_b / 2 L_b.  E0 alone
 *              also shows the look-ahead context rows conv1 reads: its live length is L_b + ctx_b
 *   tables     PE1 / PE2 / POS: out [2 T - 1, 512], T = the encoded width (W, in the partial mode W - 3) at token rate, twice that
 *              at mel rate; no batch geometry
 * One id per tap, in execution order; the eight taps of block i are the block-0 ids + JV_UPS_TAP_PER_BLOCK * i (93 ids, 0 .. 92):
 *   EMB  (512)  the embedded tokens                          EL   (512)  embed.out.0 (Linear)
 *   E0   (512)  its LayerNorm x sqrt(512)                    PE1  table  relative positions T - 1 .. -(T - 1), sin | cos interleaved
 *   C1   (512)  look-ahead conv1 + bias (LeakyReLU is conv2's prologue)
 *   LA   (512)  conv2 + bias + E0: the blocks' input
 *   per block (six at token rate from JV_UPS_TAP_LN1_0, four at mel rate from JV_UPS_TAP_ULN1_0):
 *     LN1 (512) norm_mha   QKV (1536) q | k | v   POS table linear_pos(PE)   ATT (512) the attention, ahead of linear_out
 *     X1  (512) x + linear_out(att)   LN2 (512) norm_ff   FF (2048) SiLU(w_1)   X2 (512) X1 + w_2(FF): the block's output
 *   REP  (512)  nearest x 2            UP   (512)  up_layer.conv (k5, causal)
 *   UL   (512)  up_embed.out.0         U0   (512)  its LayerNorm x sqrt(512)     PE2  table
 *   AN   (512)  after_norm             H    (80)   encoder_proj: the entry's output, here channels first */
#define JV_UPS_MODE_PROMPT 0
#define JV_UPS_MODE_FLOW 1
#define JV_UPS_MODE_PARTIAL 2
#define JV_UPS_MODE_CTX 3
#define JV_UPS_TAP_EMB 0
#define JV_UPS_TAP_EL 1
#define JV_UPS_TAP_E0 2
#define JV_UPS_TAP_PE1 3
#define JV_UPS_TAP_C1 4
#define JV_UPS_TAP_LA 5
#define JV_UPS_TAP_LN1_0 6     /* token-rate block i < 6: + JV_UPS_TAP_PER_BLOCK * i */
#define JV_UPS_TAP_QKV_0 7
#define JV_UPS_TAP_POS_0 8
#define JV_UPS_TAP_ATT_0 9
#define JV_UPS_TAP_X1_0 10
#define JV_UPS_TAP_LN2_0 11
#define JV_UPS_TAP_FF_0 12
#define JV_UPS_TAP_X2_0 13
#define JV_UPS_TAP_PER_BLOCK 8
#define JV_UPS_TAP_REP 54
#define JV_UPS_TAP_UP 55
#define JV_UPS_TAP_UL 56
#define JV_UPS_TAP_U0 57
#define JV_UPS_TAP_PE2 58
#define JV_UPS_TAP_ULN1_0 59   /* mel-rate block i < 4: the same eight, + JV_UPS_TAP_PER_BLOCK * i */
#define JV_UPS_TAP_AN 91
#define JV_UPS_TAP_H 92
#define JV_UPS_TAP_COUNT 93
int jv_upsample_encoder_tap(jv_context* ctx, int mode, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                            const int64_t* token_lens, const int32_t* ctx_lens, int B, int P, int N, int streaming, int tap,
                            float* out, int64_t out_floats, void* stream);
int jv_flow_token2mel_ctx(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                          const int64_t* token_lens, const int32_t* ctx_lens, const float* prompt_feat, const int32_t* feat_lens,
                          const float* embedding, int B, int P, int N, int F, int streaming, int n_timesteps, float temperature,
                          const float* t_span_host, float* mel, int32_t* mel_lens, void* stream);

/* jv_load_mel_basis / jv_mel_spectrogram: the prompt-mel front-end, `extract_speech_feat` of infer.py:166-186 ->
 * `mel_spectrogram` of jyutvoice/utils/audio.py:18-63 (24 kHz, n_fft = win = 1920 periodic Hann, hop 480, reflect pad 720,
 * center=False, |.| with the 1e-9 floor, 80 mel bands, log(clamp(., 1e-5))).
 * basis: the [80][961] fp32 mel filterbank (librosa.filters.mel(sr=24000, n_fft=1920, n_mels=80, fmin=0, fmax=8000) in the
 * reference -- data to this library); wav: [B, n_samples] in [-1, 1], n_samples > 720; mel: [B, 80, T],
 * T = 1 + (n_samples - 480) / 480. */
int jv_load_mel_basis(jv_context* ctx, const float* basis, int64_t numel, int on_device, void* stream);
int jv_mel_spectrogram(jv_context* ctx, const float* wav, int B, int n_samples, float* mel, void* stream);
/* jv_mel_spectrogram_ragged: the same front-end for recordings of different durations in one call -- the per-utterance loop of
 * infer.py:166-186 (the reference extracts one prompt at a time).  wav: [B, n_samples], recording b is wav[b, :wav_lens[b]]
 * (what lies behind it is not read); wav_lens: [B] int32 on the device, 720 < wav_lens[b] <= n_samples (else JV_ERR_ARG, naming
 * the recording).  The reflect padding of 720 samples is taken at each recording's own end.  mel: [B, 80, Tmax],
 * Tmax = 1 + (n_samples - 480) / 480, recording b in [:T_b], T_b = 1 + (wav_lens[b] - 480) / 480, zeros behind it;
 * mel_lens: [B] int32 on the device, receives T_b.  The STFT / mel GEMMs run on the valid frames only.  Synchronises the
 * stream once (the lengths are validated on the host). */
int jv_mel_spectrogram_ragged(jv_context* ctx, const float* wav, const int32_t* wav_lens, int B, int n_samples, float* mel,
                              int32_t* mel_lens, void* stream);

/* ---- sample-rate conversion ----------------------------------------------------------------------------------
 * The two `torchaudio.transforms.Resample(orig, new)` of infer.py:368-382 (the --ref_audio recording to 16 kHz and to 24 kHz), i.e.
 * torchaudio.functional.resample with its defaults: sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99.  Restated (unpinned:
 * torchaudio is not part of this build) with g = gcd(orig, new), o = orig / g, n = new / g:
 *   orig == new: a copy.  Otherwise base = 0.99 min(o, n), width = ceil(6 o / base), K = 2 width + o,
 *   h(tau) = (base / o) sinc(base tau) cos^2(pi base tau / 12) for |base tau| <= 6, else 0  (sinc(u) = sin(pi u) / (pi u)),
 *   tab[p][k] = h((k - width) / o - p / n), p in [0, n), k in [0, K): evaluated in fp64, rounded once to fp32,
 *   y[i n + p] = sum_{k < K} tab[p][k] x[i o + k - width], x = 0 outside [0, L), for the first ceil(n L / o) output samples;
 *   products and sum in fp32, k ascending, the same order for every sample wherever it lies in a batch.
 *
 * jv_resample_length: infer.py:368-382's output length, ceil(new n / orig) in reduced integers; n for equal rates; -1 for n < 0,
 *   a rate <= 0 or a result beyond int64.  Host only, no context.
 * jv_resample_table: the table above for a rate pair (host only, no context, no device, like jv_h3_scale_for_bound).  Writes
 *   *o, *n, *width (each optional); with tab != NULL and cap >= n K also tab[p * K + k], with tab != NULL and a smaller cap
 *   JV_ERR_SHAPE; tab == NULL queries the sizes.  Equal rates give o = n = 1 and the filter of that pair, which jv_resample does
 *   not use.  JV_ERR_ARG for a rate <= 0 or a table of more than 2^20 entries (n K; the message names o, n and the cap).
 * jv_resample: infer.py:368-382 for a ragged batch in one launch.  wav: [B, n_in]; lens: [B] int32 on the device or NULL (all n_in),
 *   clamped as under "Lengths" above: it MEANS len_b = min(max(lens[b], 0), n_in), and what lies behind it is not read (it may be
 *   NaN).  out: [B, n_out], n_out >= jv_resample_length(n_in, orig_freq, new_freq) else JV_ERR_SHAPE; recording b fills
 *   out[b, :ceil(n len_b / o)], zeros behind.  out_lens: optional [B] int32 on the device, receives ceil(n len_b / o).
 *   Rates <= 0 and reduced pairs whose table exceeds 2^20 entries: JV_ERR_ARG, before anything is launched; the context stays
 *   usable.  The table is built on the host and uploaded once per (o, n) (a small cache in the context, untouched by jv_reserve);
 *   with the table cached the call only enqueues on `stream` and never synchronises.  A miss allocates, copies synchronously and,
 *   once the cache holds 8 tables, waits for the device and frees the least recently used one.  So under stream capture: make the
 *   first call for a reduced pair (o, n) OUTSIDE the capture (a miss while capturing fails), and a context that has served more
 *   than 8 distinct reduced pairs since may have freed the table a captured launch points to -- capture again after that.
 *   One launch holds fewer than 2^24 workgroups (B ceil(n_out / tile), tile <= 1024): beyond that JV_ERR_SHAPE. */
int64_t jv_resample_length(int64_t n, int orig_freq, int new_freq);
int jv_resample_table(int orig_freq, int new_freq, float* tab, int64_t cap, int32_t* o, int32_t* n, int32_t* width);
int jv_resample(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n_in, int orig_freq, int new_freq, float* out,
                int64_t n_out, int32_t* out_lens, void* stream);

/* ---- reference-audio features at 16 kHz ---------------------------------------------------------------------
 * What infer.py:98-163 computes from the 16 kHz copy of the reference recording: the input of campplus.onnx
 * (`kaldi.fbank(speech, num_mel_bins=80, dither=0, sample_frequency=16000)` minus its mean over frames, infer.py:148-163) and the
 * input of speech_tokenizer_v2.onnx (`whisper.log_mel_spectrogram(audio, n_mels=128)`, infer.py:98-145).  Both are restated here
 * (unpinned: torchaudio and whisper are not part of this build).
 *
 * fbank.  x: len samples in [-1, 1], NOT rescaled to int16 range.  len < 400: 0 frames.  Otherwise T = 1 + (len - 400) / 160 frames,
 *   frame f = x[160 f : 160 f + 400]; per frame: subtract the frame's mean; pre-emphasis a[i] -= 0.97 a[i-1] with a[-1] := a[0];
 *   times the Povey window (0.5 - 0.5 cos(2 pi i / 399))^0.85; zero-pad to 512, |rfft|^2; 80 triangular banks equally spaced on
 *   mel(f) = 1127 ln(1 + f / 700) between mel(20) and mel(8000): bank b rises from lo + b d to lo + (b + 1) d and falls to
 *   lo + (b + 2) d, d = (hi - lo) / 81, the weight of bin k < 256 is max(0, min(up, down)) at mel(31.25 k), bin 256 has weight 0;
 *   log(max(E, 2^-23)), natural.  [T, 80]; with subtract_mean the mean over the recording's own T frames is subtracted per bin.
 * Whisper log-mel.  Reflect-pad 200 samples per side (needs len > 200); frames of 400 every 160, periodic Hann
 *   0.5 - 0.5 cos(2 pi i / 400), 400-point |rfft|^2 (201 bins); the last frame is dropped: T = len / 160 frames; the 128 x 201
 *   filterbank is data (whisper ships librosa.filters.mel(sr=16000, n_fft=400, n_mels=128); jv_load_whisper_filters);
 *   L = log10(max(E, 1e-10)); L = max(L, max(L) - 8), the maximum over that recording's whole [128, T]; (L + 4) / 4.  [128, T].
 * Arithmetic: conditioning, both products (k in a fixed order that does not depend on the frame's place in a tile or a batch),
 *   the power and the logs in fp32; windows and DFT bases evaluated in fp64 and rounded once; a recording's mean / maximum is
 *   reduced over its tiles of 32 frames in ascending order.  A recording gives the same bits alone and in any batch.
 *
 * jv_fbank_frames / jv_whisper_frames: the frame counts above for n samples (0 when too short).  Host only, no context.
 * jv_kaldi_mel_banks: the 80 x 257 bank weights above, evaluated in fp64 and rounded once.  Host only, no context.
 * jv_load_whisper_filters: the [128, 201] filterbank (host or device memory); numel != 128 * 201: JV_ERR_SHAPE.  Synchronises.
 * jv_fbank: wav [B, n]; lens: [B] int32 on the device or NULL (all n), clamped as under "Lengths" above: it MEANS
 *   len_b = min(max(lens[b], 0), n), and what lies behind it is not read (it may be NaN).  out: [B, Tmax, 80],
 *   Tmax = jv_fbank_frames(n); recording b fills out[b, :T_b], exact zeros behind.  out_lens: optional [B] int32 on the device,
 *   receives T_b.  A recording too short for a frame has T_b = 0, a zero row and no error (nothing comes down to the host, so the
 *   library cannot reject it); with lens == NULL the host knows n and returns JV_ERR_ARG for n < 400.
 * jv_whisper_log_mel: the same contract; out: [B, 128, Tmax], Tmax = jv_whisper_frames(n); too short is len <= 200.
 *   JV_ERR_STATE before jv_load_whisper_filters.
 * Every error is returned before anything is launched and leaves the context usable.  Each call is two launches on `stream`
 * (one with subtract_mean == 0) and never synchronises -- except that the first call of a feature in a context allocates its
 * window, basis and bank tables (fbank: uploads the banks synchronously), and a call with more tiles (B ceil(Tmax / 32)) than any
 * before waits for the device and re-allocates the partials buffer: under stream capture make a call of the largest shape
 * outside the capture first.  These buffers are not workspace: jv_reserve leaves them alone, jv_destroy frees them.
 * One launch holds fewer than 2^24 workgroups: beyond that JV_ERR_SHAPE. */
int64_t jv_fbank_frames(int64_t n);
int64_t jv_whisper_frames(int64_t n);
int jv_kaldi_mel_banks(float* out /* 80 * 257 */);
int jv_load_whisper_filters(jv_context* ctx, const float* data, int64_t numel, int on_device, void* stream);
int jv_fbank(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, int subtract_mean, float* out, int32_t* out_lens,
             void* stream);
int jv_whisper_log_mel(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, float* out, int32_t* out_lens,
                       void* stream);

/* ---- levels: prompt silence trim, peak, BS.1770 loudness, gain ----------------------------------------------
 * What a CosyVoice2 front-end does to a reference recording before any feature is taken (energy trim 60 dB below the loudest frame,
 * frame 440, hop 220; scale down to a peak of 0.8; append 0.2 s of silence) and the usual last step of a TTS service (programme
 * loudness after ITU-R BS.1770-4 / EBU R 128).  The reference's infer.py does neither.  All definitions are restated here
 * (unpinned: librosa, pyloudnorm and torchaudio are not part of this build).
 *
 * Energy trim: the contract of librosa.effects.trim(y, top_db, frame_length = F, hop_length = H) with zero centre padding, in the
 *   linear domain.  x[0..N) padded with F / 2 zeros per side (xp); T = 1 + (N + 2 (F / 2) - F) / H frames (0 if that is negative or
 *   N == 0); ms_t = (1 / F) sum_{i < F} xp[t H + i]^2, m_t = max(1e-10, ms_t), M = max_t m_t; frame t is non-silent iff
 *   m_t > M 10^(-top_db / 10); start = H (first non-silent t), end = min(N, H (last non-silent t + 1)); none, or N == 0:
 *   start = end = 0.  An all-zero recording has every m_t = M: nothing is trimmed.  fp32: a frame's sum is 64 interleaved fmaf
 *   chains (i mod 64, i ascending) joined by a fixed butterfly; the threshold is evaluated in fp64 and rounded once.
 * Peak: max |x| over the recording, or over [start, end) (each clamped into [0, len], end >= start); exact; 0 for an empty range.
 * Integrated loudness (mono).  K-weighting = shelf then high-pass, two biquads whose coefficients follow from the standard's
 *   48 kHz table by the usual re-derivation, evaluated in fp64: with K = tan(pi f0 / fs), a0 = 1 + K / Q + K^2,
 *   a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0] for both;
 *   shelf: f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, Vh = 10^(G / 20), Vb = Vh^0.4996667741545416,
 *     b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0];
 *   high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1].
 *   Zero state before sample 0, y = high-pass(shelf(x)).  h = (fs + 5) / 10 samples; block j covers [j h, j h + 4 h) for
 *   j < nb = (N - 4 h) / h + 1 (0 when N < 4 h); z_j = mean(y^2) over the block.  Absolute gate: z_j > 10^((-70 + 0.691) / 10);
 *   relative gate: also z_j > 0.1 mean(z over the blocks past the absolute gate); L = -0.691 + 10 log10(mean z over the blocks
 *   past both); no block, or none past the absolute gate: L = -inf (never NaN).  The recurrence and every sum run in fp64 in an
 *   order fixed by the sample index; L is rounded once to fp32.
 * Gain: g = 10^((target - L) / 20); with a ceiling c > 0 and peak given, g = min(g, c / peak); L = -inf or peak == 0: g = 1.
 *   Without lufs (the prompt rule): g = c / peak if peak > c, else 1.  Evaluated in fp64, rounded once.
 * Apply: out[b, :e - s] = x[b, s:e] g_b (one fp32 multiply), then `tail` zeros, out_lens[b] = e - s + tail, exact zeros behind.
 *
 * jv_kweight_coeffs: out = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 for a rate.  jv_loudness_blocks: nb above (-1 for a bad
 *   rate).  Both host only, no context.  Rates outside [8000, 192000]: JV_ERR_ARG.
 * Common to the five device calls: wav [B, n] fp32; lens [B] int32 on the device or NULL (all n), clamped as under "Lengths" above:
 *   it MEANS len_b = min(max(lens[b], 0), n), and what lies behind it is not read (it may be NaN); start / end / peak / lufs / gain
 *   are [B] device vectors.  Every error is returned before anything is launched and leaves the context usable; results are
 *   written to device memory and nothing comes back to the host.  A recording gives the same bits alone and in any ragged batch.
 * jv_trim_bounds: 1 <= hop_length, 1 <= frame_length <= 8192, top_db > 0 and finite, else JV_ERR_ARG.  Four launches.
 * jv_peak: start / end optional (NULL: the whole recording).  One memset and one launch.
 * jv_loudness: fs in [8000, 192000] else JV_ERR_ARG.  Four launches (segment scan, carry, bins, gates).
 * jv_level_gain: target_lufs and ceiling are doubles (0.8 means 0.8, not its fp32 neighbour); lufs == NULL is the prompt rule (needs peak and ceiling > 0, else JV_ERR_ARG); otherwise ceiling <= 0 means none,
 *   and a ceiling > 0 needs peak.
 * jv_level_apply: start / end / gain optional (NULL: 0 / len / 1); n_out >= n + tail else JV_ERR_SHAPE; tail >= 0; out_lens optional.
 * The calls only enqueue on `stream` and never synchronise -- except that jv_loudness builds and uploads two 65 x 4 x 4 tables of
 * powers of the filter's transition matrix on the first use of a sample rate (a cache of 8 rates in the context; a miss copies
 * synchronously and, once full, waits for the device and frees the least recently used), and that jv_trim_bounds / jv_loudness
 * with a larger B x n than any call before wait for the device and re-allocate their intermediates (one buffer per context: calls
 * that use it must be ordered on one stream).  So under stream capture: make a call of the largest shape and of each sample rate
 * OUTSIDE the capture first.  These buffers are not workspace: jv_reserve leaves them alone, jv_destroy frees them.
 * One launch holds at most 2^24 workgroups (8192 samples or 4 trim frames each): beyond that JV_ERR_SHAPE. */
int jv_kweight_coeffs(int fs, double* out /* 10 */);
int64_t jv_loudness_blocks(int64_t n, int fs);
int jv_trim_bounds(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, float top_db, int frame_length,
                   int hop_length, int32_t* start, int32_t* end, void* stream);
int jv_peak(jv_context* ctx, const float* wav, const int32_t* lens, const int32_t* start, const int32_t* end, int B, int n,
            float* peak, void* stream);
int jv_loudness(jv_context* ctx, const float* wav, const int32_t* lens, int B, int n, int fs, float* lufs, void* stream);
int jv_level_gain(jv_context* ctx, const float* lufs, const float* peak, int B, double target_lufs, double ceiling, float* gain,
                  void* stream);
int jv_level_apply(jv_context* ctx, const float* wav, const int32_t* lens, const int32_t* start, const int32_t* end,
                   const float* gain, int B, int n, int tail, float* out, int64_t n_out, int32_t* out_lens, void* stream);

/* ---- evaluation forward(): alignment search and the three losses (no gradients) --------------------------------
 * What JyutVoiceTTS.forward (jyutvoice_tts.py:255-364) computes between the encoder and its return, around one call of
 * jv_flow_estimator_step.  Tensors are device pointers: mu_x [B,80,Tx], h = decoder_h [B,Ty,80] (batch, time, channel), x_lens and
 * y_lens [B] int32, attn / log_prior [B,Tx,Ty] (the reference's layout), frame_index [B,Ty] int32, durations [B,Tx] int32.
 *
 * Lengths of jv_log_prior, jv_maximum_path and jv_align: 1 <= x_lens[b] <= Tx and x_lens[b] <= y_lens[b] <= Ty, else JV_ERR_ARG
 * naming the utterance, before anything is launched (the reference reads out of bounds when t_y < t_x: that case is rejected, not
 * clamped).  Both vectors come down with the call's one synchronisation.  Tx <= max_tokens, Ty <= max_frames of the context and
 * Tx <= 2048, else JV_ERR_SHAPE.  Nothing behind a length is read (it may be NaN).  jv_align_losses, jv_cfm_loss_inputs and
 * jv_masked_mse never synchronise; their lengths MEAN min(max(len, 0), T) as under "Lengths" above.
 *
 * jv_log_prior: jyutvoice_tts.py:306-314.  log_prior[b,x,y] = -0.5 sum_c (h[b,y,c] - mu_x[b,c,x])^2 - 0.5 log(2 pi) 80 for
 *   x < x_lens[b], y < y_lens[b], zeros elsewhere.  The reference expands the square into three matmuls with factor = -0.5; this is
 *   the difference form, fp32: one fused multiply-add per channel into four interleaved partial sums (c mod 4), (s0 + s1) + (s2 + s3).
 * jv_maximum_path: monotonic_align.maximum_path (utils/monotonic_align/__init__.py:7-22, core.pyx:11-37) on the device.  value:
 *   [B,Tx,Ty] scores.  The recurrence of core.pyx:19-32 in fp32 (max_neg_val = -1e9, one add per cell) and the backtrack of
 *   core.pyx:34-37 with its tie rule (`<`, strict: equal scores stay on the same token).  attn (optional): fp32 one-hot path, zeros
 *   outside the utterance; frame_index: the token of every frame, -1 behind y_lens[b]; durations (optional): frames per token, 0
 *   behind x_lens[b].  One workgroup per utterance; no workgroup waits for another.
 * jv_align: jv_log_prior + jv_maximum_path from mu_x and h without the [B,Tx,Ty] round trip; log_prior is optional.
 * jv_align_losses: logw [B,1,Tx] ->
 *   dur_loss   = sum((logw - log(1e-8 + durations) * x_mask)^2) / sum(x_lens)          (utils/model.py:49-51, jyutvoice_tts.py:321-322)
 *                summed over x < x_lens[b]: the reference's logw is masked by the duration predictor, so its terms behind the
 *                length are zeros; logw, durations, mu_x, h and frame_index are not read behind their lengths
 *   mu_y[b,:,y] = mu_x[b,:,frame_index[b,y]], zeros behind y_lens[b]: [B,80,Ty]         (jyutvoice_tts.py:334-335, the one-hot matmul)
 *   prior_loss = sum(0.5 ((h - mu_y)^2 + log(2 pi)) * y_mask) / (sum(y_lens) * 80)     (jyutvoice_tts.py:349-362)
 *   dur_loss, prior_loss: one device float each.
 * jv_cfm_loss_inputs: the estimator inputs of ConditionalCFM.compute_loss (flow_matching.py:319-334) and the condition prefix of
 *   jyutvoice_tts.py:325-330.  x1 = y, z, mu_y: [B,80,T]; t: [B], already cosine-warped; cfg_mask: [B] floats 0 / 1; cond_index: [B]
 *   int32 k_b; spks: [B,80].  y_t = (1 - (1 - 1e-6) t) z + t x1; u = x1 - (1 - 1e-6) z; mu_masked = mu_y m; spks_masked = spks m;
 *   cond[b,:,:k_b] = x1[b,:,:k_b] m, zeros behind k_b.  Each product and sum rounded on its own, as the reference's tensor ops are.
 * jv_masked_mse: F.mse_loss(a * mask, b * mask, reduction="sum") / (sum(mask) * C) of flow_matching.py:337-339; a, b: [B,C,T], mask
 *   from lens; out: one device float.
 * Reductions are per-workgroup partials added in a fixed order by one finishing launch: no float atomics, the same bits every run.
 * The search's score buffer ([B,Ty,Tx]), its decision bits, the partials and a pinned length vector belong to the context and grow
 * on demand (a call larger than any before waits for the device and re-allocates: under stream capture make the largest call
 * outside the capture first).  They are not workspace: jv_reserve leaves them alone, jv_destroy frees them. */
int jv_log_prior(jv_context* ctx, const float* mu_x, const float* h, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty,
                 float* log_prior, void* stream);
int jv_maximum_path(jv_context* ctx, const float* value, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty, float* attn,
                    int32_t* frame_index, int32_t* durations, void* stream);
int jv_align(jv_context* ctx, const float* mu_x, const float* h, const int32_t* x_lens, const int32_t* y_lens, int B, int Tx, int Ty,
             float* log_prior, float* attn, int32_t* frame_index, int32_t* durations, void* stream);
int jv_align_losses(jv_context* ctx, const float* logw, const int32_t* durations, const int32_t* x_lens, const float* mu_x, const float* h,
                    const int32_t* frame_index, const int32_t* y_lens, int B, int Tx, int Ty, float* mu_y, float* dur_loss,
                    float* prior_loss, void* stream);
int jv_cfm_loss_inputs(jv_context* ctx, const float* x1, const float* z, const float* t, const float* cfg_mask, const int32_t* cond_index,
                       const float* mu_y, const float* spks, int B, int T, float* y_t, float* u, float* mu_masked, float* spks_masked,
                       float* cond, void* stream);
int jv_masked_mse(jv_context* ctx, const float* a, const float* b, const int32_t* lens, int B, int C, int T, float* out, void* stream);

/* ---- text encoder + duration predictor + length regulation ---------------------------------------------
 * jv_encoder_fwd: spk_embed_affine_layer(normalize(spk)) + TextEncoder.forward + DurationPredictor.forward
 * (jyutvoice/models/jyutvoice_tts.py:175-182, text_encoder.py:406-451, duration_predictor.py:48-60).
 * ids: int64 [B,Tt] each; x_lengths: int64 [B]; spk: [B,192] (raw, un-normalised).
 * outputs: x [B,576,Tt], mu_x [B,80,Tt], logw [B,1,Tt], spks_proj [B,80].
 * Tt is bounded by the max_tokens of jv_create / jv_reserve alone; which attention kernels run is jv_encoder_set_attention's. */
int jv_encoder_fwd(jv_context* ctx, const int64_t* phone, const int64_t* lang, const int64_t* tone, const int64_t* word_pos,
                   const int64_t* syllable_pos, const int64_t* x_lengths, const float* spk, int B, int Tt, float* x,
                   float* mu_x, float* logw, float* spks_proj, void* stream);
/* jv_encoder_fwd_tap (used by the parity tests): jv_encoder_fwd's own launch sequence up to and including one stage, whose
 * workspace buffer is then copied out channels-first as out [B, C, Tt] -- an early return inside the function jv_encoder_fwd runs
 * (the prenet buffers ping-pong and the hidden state is updated in place, so a stage can only be read where it stands), not a
 * second sequence: the route decision, the row mask and every launch ahead of the return are the whole forward's.  Outputs whose
 * launches lie behind the tap are not written (logw never; x and mu_x only by XD, D1, D2; spks_proj, the first stage, always).  Positions at or behind an utterance's clamped length are zeros.
 * out_floats < B*C*Tt: JV_ERR_SHAPE; an unknown tap: JV_ERR_ARG; both before the first launch.  One id per tap, in execution
 * order; the five taps of encoder layer i are the layer-0 ids + JV_ENC_TAP_PER_LAYER * i (38 ids, 0 .. 37).  Taps (C):
 *   EMB   (192)   the four embeddings' sum x sqrt(192)
 *   PREk  (192)   behind the k-th prenet conv k5 + channel LayerNorm + ReLU, k = 0 .. 2
 *   H0    (576)   prenet projection + residual, masked | raw speaker vector | language embedding: the layers' input
 *   QKVi  (1728)  q | k | v of layer i, RoPE applied to q and k
 *   ATTi  (576)   the attention's output, ahead of conv_o
 *   N1i   (576)   LayerNorm 1 of (h + conv_o(att))
 *   FFi   (768)   ReLU(conv_1)
 *   N2i   (576)   LayerNorm 2 of (h + conv_2(ff)): the layer's output
 *   XD    (576)   x + cond(spk): the duration predictor's input
 *   D1, D2 (256)  behind each of its conv k3 + ReLU + LayerNorm */
#define JV_ENC_TAP_EMB 0
#define JV_ENC_TAP_PRE0 1    /* PRE1 = 2, PRE2 = 3 */
#define JV_ENC_TAP_H0 4
#define JV_ENC_TAP_QKV0 5    /* layer i: + JV_ENC_TAP_PER_LAYER * i */
#define JV_ENC_TAP_ATT0 6
#define JV_ENC_TAP_N10 7
#define JV_ENC_TAP_FF0 8
#define JV_ENC_TAP_N20 9
#define JV_ENC_TAP_PER_LAYER 5
#define JV_ENC_TAP_XD 35
#define JV_ENC_TAP_D1 36
#define JV_ENC_TAP_D2 37
int jv_encoder_fwd_tap(jv_context* ctx, const int64_t* phone, const int64_t* lang, const int64_t* tone, const int64_t* word_pos,
                       const int64_t* syllable_pos, const int64_t* x_lengths, const float* spk, int B, int Tt, float* x,
                       float* mu_x, float* logw, float* spks_proj, int tap, float* out, int64_t out_floats, void* stream);
/* jv_encoder_set_attention: the route of the encoder layers' 2-head RoPE attention (text_encoder.py:216-248) in jv_encoder_fwd.
 *   JV_ENC_ATTN_AUTO (default): the four-launch route (q k^T GEMM, masked softmax, V transpose, P V GEMM around a [B,2,Tt,Tt] score
 *                        buffer) for Tt <= 512, the one-launch kernel of encattn.hip above that
 *   JV_ENC_ATTN_FUSED:   encattn.hip at every length
 *   JV_ENC_ATTN_GEMM:    the four-launch route; jv_encoder_fwd with Tt > 512 returns JV_ERR_SHAPE
 * Another value: JV_ERR_ARG, and the mode stays as it was.  The workspace holds the score buffer for min(max_tokens, 512) tokens. */
#define JV_ENC_ATTN_AUTO 0
#define JV_ENC_ATTN_FUSED 1
#define JV_ENC_ATTN_GEMM 2
int jv_encoder_set_attention(jv_context* ctx, int mode);
/* jv_length_regulate: w_ceil = ceil(exp(logw)*mask)*length_scale, y_lengths, generate_path, mu_y = attn^T mu_x
 * (jyutvoice_tts.py:184-203, utils/model.py:29-46).  Two-phase because T_max is data dependent:
 *   phase 1 (attn == NULL): writes w_ceil [B,1,Tt] and y_lengths [B] int64 (device); the caller reads max(y_lengths)
 *   phase 2: writes attn [B,Tt,Ty] (dense 0/1 path) and mu_y [B,80,Ty] for the given Ty. */
int jv_length_regulate(jv_context* ctx, const float* logw, const int64_t* x_lengths, const float* mu_x, int B, int Tt,
                       float length_scale, float* w_ceil, int64_t* y_lengths, int Ty, float* attn, float* mu_y,
                       void* stream);

/* ---- HiFT vocoder -------------------------------------------------------------------------------------------
 * jv_hift_f0:     ConvRNNF0Predictor.forward (jyutvoice/hifigan/f0_predictor.py:52-55): mel [B,80,T] -> f0 [B,T]
 * jv_hift_source: f0_upsamp + SourceModuleHnNSF/SineGen (generator.py:459-461, 141-176, 220-236) with the random
 *                 draws supplied: phase [B,9] (harmonic 0 ignored, treated as 0), noise [B,9,480T] ~ N(0,1);
 *                 -> s [B,1,480T]
 * jv_hift_decode: HiFTGenerator.decode (generator.py:396-432): mel [B,80,T], s [B,1,480T] -> wav [B,480T]
 * lens: [B] int32 valid mel frames per utterance or NULL ("Lengths" above: clamped to [0, T]; wav is zero behind 480 lens[b]). */
int jv_hift_f0(jv_context* ctx, const float* mel, const int32_t* lens, int B, int T, float* f0, void* stream);
int jv_hift_source(jv_context* ctx, const float* f0, const float* phase, const float* noise, int B, int T, float* s,
                   void* stream);
/* jv_hift_source_seeded: the same with the noise drawn INSIDE the kernel -- generator.py:171 (`torch.randn_like`) draws
 * values no caller can depend on, and a [B,9,480T] tensor written by one kernel only to be read once by the next is 166 MB
 * per pass at the headline size.  Each sample's nine N(0,1) draws are Philox4x32-10 + Box-Muller of (seed, call, utterance,
 * sample): reproducible for a given (seed, call), independent across calls (the caller counts them).  Parity tests inject the
 * oracle's noise through jv_hift_source instead. */
int jv_hift_source_seeded(jv_context* ctx, const float* f0, const float* phase, uint64_t seed, uint32_t call, int B, int T, float* s,
                          void* stream);
/* jv_hift_source_cont: jv_hift_source_seeded for a signal that arrives in pieces.  This call writes samples sample0 ..
 * sample0 + 480 T - 1 from the f0 of the next T frames; `cum` [B,9] doubles (device, 8-byte aligned) carries the sine generator's
 * running phase sums from call to call -- all zeros before the first piece, read and updated on the stream, no host round trip --
 * and the noise counters use the absolute sample index.  Over any split of an f0 array into consecutive pieces the concatenated
 * output equals jv_hift_source_seeded on the whole array with the same (phase, seed, call) bit for bit: the frame scan is a
 * sequential fp64 recurrence that simply resumes, and a sample is a pure function of (its frame's start sum, f0, index). */
int jv_hift_source_cont(jv_context* ctx, const float* f0, const float* phase, uint64_t seed, uint32_t call, int64_t sample0, double* cum,
                        int B, int T, float* s, void* stream);
/* jv_hift_source_cont_rows: jv_hift_source_cont with every row an independent signal -- the sessions of a streaming server in one
 * launch.  seeds, calls, sample0, lens: [B] on the device (seeds, sample0 and cum 8-byte aligned).  Row b's noise is keyed by
 * seeds[b] and counted (sample0[b] + n, utterance 0, calls[b]); its frame scan resumes from cum[b] over lens[b] frames (clamped
 * to [0, T]) and leaves the sums after exactly those frames in cum[b]; s[b] is zeros behind 480 lens[b].  A row with lens[b] = 0 is
 * not touched: neither s[b] nor cum[b] is written.  Row b equals jv_hift_source_cont at B = 1 with that row's scalars and its first
 * lens[b] frames bit for bit, whichever slot it sits in. */
int jv_hift_source_cont_rows(jv_context* ctx, const float* f0, const float* phase, const uint64_t* seeds, const uint32_t* calls,
                             const int64_t* sample0, const int32_t* lens, double* cum, int B, int T, float* s, void* stream);
/* jv_slab_copy: B column slabs between two [rows, C, width] fp32 buffers in one launch -- the state moves of a batch of streaming
 * sessions (append, window gather, crop).  desc: [B, 5] int32 on the device, (src_row, src_col, dst_row, dst_col, n):
 * dst[dst_row, :, dst_col + j] = src[src_row, :, src_col + j] for j < n <= span and, with zero_fill != 0, zero for n <= j < span
 * (cut at dst_width).  A descriptor that does not fit its buffers, or whose n is negative or above span, moves nothing.  The
 * buffers must not overlap; slabs of one call must not overlap in the destination.  Owns no memory and uses none of the
 * workspace: what a caller keeps in such buffers survives jv_reserve. */
int jv_slab_copy(jv_context* ctx, const float* src, int src_rows, int src_width, float* dst, int dst_rows, int dst_width, int C,
                 const int32_t* desc, int B, int span, int zero_fill, void* stream);
int jv_hift_decode(jv_context* ctx, const float* mel, const float* s, const int32_t* lens, int B, int T, float* wav,
                   void* stream);
/* jv_hift_decode_tap (used by the parity tests): jv_hift_decode's own launch sequence up to and including one stage, whose
 * workspace buffer is then copied out channels-first as out [B, C, L] -- an early return inside the function jv_hift_decode
 * runs, not a second sequence: the geometry decision, the masks and every launch ahead of the return are the whole decode's.
 * No waveform is written.  Positions at or behind an utterance's clamped length (lens[b] frames = L-per-frame x lens[b]
 * positions, + 1 at the x120 level) are zeros, an utterance of length 0 is all zeros.  out_floats < B*C*L: JV_ERR_SHAPE;
 * an unknown tap: JV_ERR_ARG; both before the first launch.  Taps in execution order (C, L):
 *   STFT   (18, 120 T + 1)  9 real | 9 imaginary bins of the source's 16-point STFT
 *   PRE    (512, T)         conv_pre
 *   UPi    (256, 8 T) / (128, 40 T) / (64, 120 T + 1)   the i-th ConvTranspose1d (i = 2: behind the reflection pad)
 *   SIi    as UPi           the i-th source-down convolution, ahead of its ResBlock
 *   XSi    as UPi           UPi + the source ResBlock
 *   Xi     as UPi           the mean of the three ResBlocks (the stage's output)
 *   POST   (18, 120 T + 1)  conv_post: 9 log-magnitudes | 9 phases
 *   FRAMES (16, 120 T + 1)  the windowed inverse-DFT frames, ahead of overlap-add and clip */
#define JV_HIFT_TAP_STFT 0
#define JV_HIFT_TAP_PRE 1
#define JV_HIFT_TAP_UP0 2    /* UP1 = 3, UP2 = 4 */
#define JV_HIFT_TAP_SI0 5    /* SI1 = 6, SI2 = 7 */
#define JV_HIFT_TAP_XS0 8    /* XS1 = 9, XS2 = 10 */
#define JV_HIFT_TAP_X0 11    /* X1 = 12, X2 = 13 */
#define JV_HIFT_TAP_POST 14
#define JV_HIFT_TAP_FRAMES 15
int jv_hift_decode_tap(jv_context* ctx, const float* mel, const float* s, const int32_t* lens, int B, int T, int tap, float* out,
                       int64_t out_floats, void* stream);

/* ---- operator-level entry points (used by the parity tests; same kernels the stages above launch) -------------
 * jv_op_conv_gemm: out[m,n] = act(sum_{j,ci} A[m + tap_row0 + j*dil, ci] * W[n, j*Cin + ci] + bias[n]) (+ res[m,n])
 *                  A [a_rows, Cin] rows, W [N, ntaps*Cin], optional LayerNorm over N (N == 256) before act.
 * jv_op_attention: softmax(q k^T / 8 over keys < lens[b]) v for qkv rows [G + b*S + t][1536], 8 heads x 64.
 * jv_op_layernorm: rows [rows, C].
 * jv_op_linear_h3: out = act(A W^T + bias) (+ res) through the fp16x3 main loop (jv_flow_set_contraction); A [rows, K],
 *                  W [N, K], a_bound = the caller's bound on |A| (the kernel's contract: |A| <= a_bound); presplit = 1:
 *                  A is first written as fp16 planes (what LayerNorm / attention / the GELU epilogue do in the estimator)
 *                  and both operands travel by LDS-DMA; 2: reuse the previous call's planes (timing only).
 * jv_op_attention_h3: jv_op_attention through the fp16x3 kernel, with the caller's bounds on |q|, |k|, |v|.
 * jv_op_conv_h3_measured: jv_op_conv_gemm through the fp16x3 main loop with a bound measured on the device: amax_in points
 *                  at a float >= max |A| (the amax_out of A's producer), a_extra bounds what the prologue adds; amax_out
 *                  (optional, zero it first) receives max |out|.  amax_in = NULL: bf16x6, tracking only. */
int jv_op_conv_gemm(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, int dil, const float* W, int N,
                    const float* bias, int act, int prologue, const float* alpha, float slope, const float* ln_g,
                    const float* ln_b, float ln_eps, const uint8_t* rowmask, const float* res, float* out, void* stream);
int jv_op_attention(const float* qkv, const int32_t* lens, int B, int G, int S, int L, float* out, void* stream);
/* jv_op_rel_attention: the conformer block's relative-position attention (attention.py:204-334) on caller-supplied buffers.
 * qkv [rows,1536] rows G + b*S + t; p = linear_pos(pos_emb) [2T-1,512]; u, v: pos_bias_u / pos_bias_v [8,64]; lens: int64 [B],
 * utterance b has min(lens[b] * len_mul, T) rows.  For head h, query i, key j:
 *   s = ((q_i + u_h) . k_j + (q_i + v_h) . p_h[T-1-i+j]) / 8  over keys j < min(L_b, (i / chunk + 1) * chunk)  (chunk = 0: j < L_b),
 * out[row(b,i), h*64 ..] = softmax_j(s) V; rows L_b <= i < T are written as zeros.  fused = 1: relattn.hip, one launch, online
 * softmax, nothing quadratic in memory; fused = 0: the three-GEMM sequence jv_prompt_encoder_fwd runs (temporaries allocated and
 * freed inside the call, which then synchronises). */
int jv_op_rel_attention(const float* qkv, const float* p, const float* u, const float* v, const int64_t* lens, int B, int T, int G,
                        int S, int len_mul, int chunk, int fused, float* out, void* stream);
/* jv_op_enc_attention: the text encoder's attention (text_encoder.py:235-248: scores, mask, softmax, P V; RoPE already applied) on
 * caller-supplied buffers.  qkv [rows,1728] rows G + b*S + t, q of head h at columns h*288, k at 576 + h*288, v at 1152 + h*288;
 * lens: int64 [B], utterance b has L_b = min(lens[b], T) rows.
 *   out[row(b,i), h*288 ..] = softmax_j(q_i . k_j / sqrt(288)) V  over keys j < L_b, for queries i < L_b  ([rows,576])
 * fused = 1: encattn.hip, one launch; rows L_b <= i < T are written as zeros, nothing at or behind L_b is read.  fused = 0: the
 * four-launch sequence of jv_encoder_fwd (temporaries allocated and freed inside the call, which then synchronises), which reads
 * all T rows and leaves the average of V in rows L_b <= i < T; T > 512: JV_ERR_SHAPE.  Rows of no utterance are not written. */
int jv_op_enc_attention(const float* qkv, const int64_t* lens, int B, int T, int G, int S, int fused, float* out, void* stream);
float jv_h3_scale_for_bound(float bound);   /* host only: the power of two chosen for a proven bound (0 = unusable) */
/* process-wide (the jv_op_* hooks take no context): fp16x3 products per step of the hooks jv_op_linear_h3,
 * jv_op_conv_h3_measured, jv_op_splitk, jv_op_attention_h3, jv_op_attention_planes, jv_op_rowgemm, jv_op_rowgemm_qkv, jv_op_rowconv,
 * jv_op_rowres and jv_op_rowblock -- 3 (default), or 1 = the hi x hi product alone, what JV_PRECISION_FP16 selects on a context.  Read by those
 * hooks and by nothing on the production path. */
int jv_op_set_products(int np);
int jv_op_conv_h3_measured(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, int dil, const float* W,
                           int N, const float* bias, int act, int prologue, const float* alpha, float slope,
                           const uint8_t* rowmask, const float* res, const float* amax_in, float a_extra, float* amax_out,
                           float* out, void* stream);
/* jv_op_splitk: a contraction to 256 channels on the estimator's short-batch route (2048 rows or fewer): split-K tiles
 * (ConvGemmArgs::ksplit) into partial sums, then ONE row-wise launch that sums them and runs the whole tail -- through the launcher
 * the estimator itself calls (conv_splitk).  N must be 256.
 *   v      = sum_j A[m + tap_row0 + j] W_j + bias                 A [a_rows, Cin] (rows with rowmask == 0 read as zero), W [256, ntaps Cin]
 *   v      = act(LayerNorm_256(v) ln_g + ln_b), eps 1e-5          (ln_g != NULL; else act alone); rows with rowmask == 0 := 0
 *   out[m] = v + rowvec[row_sample[m] * rowvec_ld] + res[m]       out [M, ldo], res [M, ldr] (may be out itself)
 *   out2[m] = LayerNorm_256(out[m]) ln2_g + ln2_b                 (ln2_g != NULL) [M, 256]
 * rowmask [a_rows] (optional) is the input mask, the output mask and the tracking mask; row_sample [a_rows]: a row's utterance.
 * ksplit_max workgroups per tile, clamped to Cin / 32 (the estimator: 8).  mode: 0 bf16x6; 1 fp16x3 scaled per utterance by the
 * measured bounds amax_in[slot_nb], slot(row) = clamp((row - slot_G) / slot_S, 0, slot_nb - 1) or, slot_S < 0, row_sample[row];
 * 2 fp16x3 scaled by the caller's proven a_bound.  amax_out [slot_nb] (optional, zero it first): max |out| over the rows with
 * rowmask != 0 is folded into slot row_sample[row]. */
int jv_op_splitk(const float* A, int64_t a_rows, int M, int Cin, int ntaps, int tap_row0, const float* W, int N, const float* bias,
                 const float* ln_g, const float* ln_b, int act, const uint8_t* rowmask, const float* rowvec,
                 const int32_t* row_sample, int rowvec_ld, const float* res, int64_t ldr, float* out, int64_t ldo, const float* ln2_g,
                 const float* ln2_b, float* out2, int ksplit_max, int mode, const float* amax_in, float a_bound, int slot_G,
                 int slot_S, int slot_nb, float* amax_out, void* stream);
int jv_op_attention_h3(const float* qkv, const int32_t* lens, int B, int G, int S, int L, float q_bound, float k_bound,
                       float v_bound, float* out, void* stream);
int jv_op_linear_h3(const float* A, int64_t rows, int M, int K, const float* W, int N, const float* bias, int act,
                    const float* res, float a_bound, int presplit, float* out, void* stream);
/* jv_op_rowgemm: the row-owning fp16x3 GEMM the estimator's transformer linears run on at batch sizes that fill the chip
 * (transformer.py:355-443), with each epilogue: epi 0 plain -> out fp32 [M,N]; 1 exact GELU -> out2 = fp16 planes
 * [2][M][N] of value * out2_scale; 2 + res -> out; 3 + res -> out, then LayerNorm_256 -> out2 = planes [2][M][256].
 * a_bound: the caller's bound on |A|; presplit = 2 reuses the previous call's A planes (timing).  N % 256 == 0, K % 32 == 0. */
int jv_op_rowgemm(const float* A, int64_t rows, int M, int K, const float* W, int N, const float* bias, int epi,
                  const float* res, const float* ln_g, const float* ln_b, float a_bound, float out2_scale, int presplit,
                  float* out, uint16_t* out2, float* amax_out, void* stream);
/* jv_op_attention_planes: the estimator's attention kernel at chip-filling batch sizes (attention_pl.hip: K / V taken as
 * fp16 planes by LDS-DMA, transposed LDS reads for V) on an fp32 qkv matrix [rows,1536]; chunk > 0: chunk-causal mask;
 * out2 != NULL: result as fp16 planes [2][rows][512] of value * out2_scale, else fp32 rows in out [rows,512]. */
int jv_op_attention_planes(const float* qkv, int64_t rows, const int32_t* lens, int B, int G, int S, int L, float q_bound,
                           float k_bound, float v_bound, int chunk, float out2_scale, float* out, uint16_t* out2, void* stream);
/* jv_op_hiftconv: the vocoder's ResBlock convolution (hiftconv_kernel.h; jyutvoice/hifigan/generator.py:90-97):
 * out = ((Conv1d(C, C, ntaps, dilation dil, same padding)(Snake_alpha(A)) + bias) + res1 + res2) * out_scale (+ out when
 * accumulate) on a [rows, C] row buffer, C = 64 / 128 / 256, W [C][ntaps * C] tap-major, rows with rowmask == 0 read as zero;
 * amax_in: slot_nb device floats, each >= max |A| over its utterance's rows, slot(row) = clamp((row - slot_G) / slot_S, 0,
 * slot_nb - 1) or, slot_map != NULL, slot_map[row] (as in jv_op_hiftpair); slot_G = slot_S = 0, slot_nb = 1, slot_map = NULL:
 * one slot for every row.  a_extra: max 1 / (alpha + 1e-9); amax_out (optional, slot_nb floats): max |out| over the rows
 * with rowmask != 0 is folded into the row's slot. */
int jv_op_hiftconv(const float* A, int64_t rows, int C, int ntaps, int dil, const float* W, const float* bias, const float* alpha,
                   const uint8_t* rowmask, const float* res1, const float* res2, float out_scale, int accumulate,
                   const float* amax_in, float a_extra, int slot_G, int slot_S, int slot_nb, const int32_t* slot_map,
                   float* amax_out, float* out, void* stream);
/* jv_hift_lds_bytes: host only, no device needed.  The dynamic LDS one workgroup of the vocoder's row-owning ResBlock kernels
 * asks for: pair = 0 hiftconv_kernel<C, NG>, pair = 1 hiftpair_kernel<C, NG, ntaps>, NG = row groups of 80 rows per workgroup;
 * -1 where the library has no such instantiation. */
int jv_hift_lds_bytes(int pair, int C, int NG, int ntaps, int dil);
/* jv_op_rowconv: the estimator's causal k = 3 convolution to 256 channels at chip-filling batch sizes (rowconv_kernel.h):
 * out[m] = tail(sum_j A[m - 2 + j] W_j + bias), tail = LayerNorm_256 (ln_g != NULL) -> act -> rows with rowmask == 0 := 0 ->
 * + rowvec (one [256] vector here) -> + res; A's fp16x3 scale comes from *amax_in (>= max |A|), amax_out receives max |out|
 * over the unmasked rows (decoder.py:110-115, 767-788). */
int jv_op_rowconv(const float* A, int64_t rows, int M, int Cin, const float* W, const float* bias, const float* ln_g,
                  const float* ln_b, int act, const uint8_t* rowmask, const float* rowvec, const float* res,
                  const float* amax_in, float* amax_out, float* out, void* stream);
int jv_op_layernorm(const float* x, const float* g, const float* b, float eps, int64_t rows, int C, float* out,
                    void* stream);
/* ---- the fused row-owning launches, from fp32 operands (tests/test_gpu_fused_ops.py).  Each hook splits its operands into fp16
 * planes, packs the weights (planes, column scales, fragment order, the registry's concatenated streams) with the library's own
 * load-time routines and calls the production launcher.  *_bound: the caller's proven bound on a tensor; the plane scale is
 * jv_h3_scale_for_bound(bound), so planes come back as value * that scale.
 *
 * jv_op_rowgemm_qkv: rowgemm's q | k | v epilogue.  A [rows, K] fp32 -- or A2, planes [2][rows][K] a producer wrote with the
 * scale of a_bound --, W [1536, K]; q fp32 [rows, 512], kv2 planes [2][rows][1024] (k in columns 0..511, v in 512..1023);
 * nsplit: column chunks over 1, 2, 3 or 6 workgroups per row tile; rt: tile height in 16-row units, 2 .. 5, 0 = the library's. */
int jv_op_rowgemm_qkv(const float* A, const uint16_t* A2, int64_t rows, int M, int K, const float* W, float a_bound, float k_bound,
                      float v_bound, int nsplit, int rt, float* q, uint16_t* kv2, void* stream);
/* jv_op_rowres: a whole CausalResnetBlock1D (decoder.py:98-115, 767-795; rowres_kernel.h) in one launch:
 *   h2  = Mish(LayerNorm1(conv3_causal(x * mask) + b1)) * mask + temb
 *   out = Mish(LayerNorm2(conv3_causal(h2 * mask) + b2)) * mask + (Wr (x * mask) + br)
 * x [rows, Cin], Cin = 256 / 512; W1 [256, 3 Cin], W2 [256, 768] tap-major (tap j reads row m - 2 + j), Wr [256, Cin]; temb [256].
 * amax_in: per-utterance bounds of x, slot(row) = clamp((row - slot_G) / slot_S, 0, slot_nb - 1) or, slot_S < 0, row_slot[row];
 * amax_out: max |out| over the unmasked rows is folded into the row's slot.  lnf_g / lnf_b (optional): the following block's
 * LayerNorm1 of the stored row -> lnf_out, planes [2][rows][256]; with Wq [1536, 256] its q | k | v instead (q, kv2 as in
 * jv_op_rowgemm_qkv).  out must not be x: the launch reads neighbouring rows as halo (JV_ERR_ARG, nothing is launched). */
int jv_op_rowres(const float* x, int64_t rows, int M, int Cin, const uint8_t* rowmask, const float* amax_in, int slot_G, int slot_S,
                 int slot_nb, const int32_t* row_slot, const float* W1, const float* b1, const float* ln1_g, const float* ln1_b,
                 const float* Wr, const float* br, const float* temb, const float* W2, const float* b2, const float* ln2_g,
                 const float* ln2_b, const float* lnf_g, const float* lnf_b, float lnf_bound, uint16_t* lnf_out, const float* Wq,
                 float k_bound, float v_bound, float* q, uint16_t* kv2, float* amax_out, float* out, void* stream);
/* jv_op_hiftpair: a vocoder ResBlock's convolution pair (generator.py:90-97; hiftpair_kernel.h) in one launch:
 *   out = ((Conv1d_k(Snake_alpha2(Conv1d_k,dil(Snake_alpha1(A)) + b1)) + b2) + A + res2) * out_scale (+ out when accumulate)
 * on a [rows, C] row buffer, C = 64 / 128, ntaps = 3 / 7 / 11, (ntaps - 1) dil <= 56, "same" padding; rows with rowmask == 0 read
 * as zero as A and as the intermediate.  amax_in: per-utterance bounds of A (slots as in jv_op_rowres, or slot_map[row]);
 * amax_out: max |out| over the unmasked rows per slot.  out must not be A. */
int jv_op_hiftpair(const float* A, int64_t rows, int C, int ntaps, int dil, const float* W1, const float* b1, const float* alpha1,
                   const float* W2, const float* b2, const float* alpha2, const uint8_t* rowmask, const float* amax_in, int slot_G,
                   int slot_S, int slot_nb, const int32_t* slot_map, const float* res2, float out_scale, int accumulate,
                   float* amax_out, float* out, void* stream);
/* jv_op_rowblock: the tail of a BasicTransformerBlock and the head of the next (transformer.py:355-443; rowblock_kernel.h):
 *   h += Wo att + bo;  out = h + W2 gelu(W1 LayerNorm3(h) + b1) + b2;  [x' = LayerNorm1_next(out);  q | k | v = Wq x']
 * mode 0: no x'; 1: x' as planes [2][rows][256] to ln_out; 2: q | k | v (out must be h); 3: the feed-forward alone (rowffn): `att`
 * is then x [rows, 256], the LayerNorm3 output, h the residual, ln1_g != NULL asks for x' in ln_out.  att [rows, 512],
 * h [rows, 256] (updated in place), out [rows, ldo] (h itself, or a separate buffer).  fused 1: one launch; 0: rowgemm<res,ln> +
 * rowffn + rowgemm<qkv> on the same plane buffers; -1: the feed-forward as rowgemm<gelu> + rowgemm<res[,ln]> as well.
 * amax_h / amax_out: max |h| / |out| over the rows with row_mask != 0, per row_slot[row].  Row buffers hold whole tiles. */
int jv_op_rowblock(const float* att, float* h, int64_t rows, int M, int mode, int fused, float att_bound, const float* Wo,
                   const float* bo, const float* ln3_g, const float* ln3_b, float ln3_bound, const float* W1, const float* b1,
                   float hid_bound, const float* W2, const float* b2, const float* ln1_g, const float* ln1_b, float ln1_bound,
                   const float* Wq, float k_bound, float v_bound, float* out, int64_t ldo, uint16_t* ln_out, float* q, uint16_t* kv2,
                   float* amax_h, float* amax_out, const int32_t* row_slot, const uint8_t* row_mask, void* stream);

/* ---- measurement -------------------------------------------------------------------------------------------
 * HIP events on the launch stream around every conv_gemm / attention launch (replaces nothing in the reference,
 * whose only timing is the unsynchronised wall clock of jyutvoice_tts.py:171-172,243-244).
 * jv_profile_report synchronises the device and writes {"kernel":{"launches":n,"ms":t,"flops":f,"bytes":b},...}. */
int jv_profile_enable(int on);
int jv_profile_report(char* json, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* JYUTVOICE_HIP_H */
