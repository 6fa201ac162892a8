// Prompt (voice-cloning) branch: FlowEncoder of the reference's infer.py:35-83 -- speech tokens [B,Tk] -> prompt_h
// [B, 2*Tk, 80] -- on row buffers.  jyutvoice/transformer/upsample_encoder.py:329-375 (forward), :20-61 (Upsample1D),
// :64-134 (PreLookaheadLayer), subsampling.py:84-115, embedding.py:201-296, encoder_layer.py:241-319,
// attention.py:204-334 (relative-position attention, rel_shift), positionwise_feed_forward.py:47-55.
//
// Two stages of the same shape: T1 = Tk rows per utterance (6 blocks), then T2 = 2*Tk rows (4 blocks).  Every Linear /
// Conv1d is the conv_gemm kernel on the bf16x6 path; the 8 x 64 relative-position attention is three batched fp32-MFMA GEMMs
// ((q + u) K^T, (q + v) P^T, softmax V) around one rel-shift + masked-softmax kernel -- the stage is ~2 % of a prompted
// synthesis, so no dedicated attention kernel is tuned for it (same choice as the text encoder, encoder.hip).
// Batches are per-utterance loops of the B = 1 reference: rows at and beyond an utterance's length are zero for the
// look-ahead / upsampling convolutions (select-zero row mask) and masked as attention keys.
//
// The same two stages serve CausalMaskedDiffWithXvec.inference (flow/flow.py:300-358, flow_encoder_fwd below), where the encoder
// runs over the WHOLE utterance [prompt tokens | tokens] in the text encoder's place: there the attention is relattn.hip's single
// launch (no [T, T] buffer in that route's workspace) and `streaming` sets the chunk masks of upsample_encoder.py:338-367.
//
// Partial sequences (flow.py:327-336, what `finalize=False` intends; jv_flow_token2mel_partial): the last ctx = 3 tokens are embedded
// like the others (upsample_encoder.py:446-453) but are only the look-ahead convolution's right context, in place of its zero padding
// (upsample_encoder.py:110-121).  They sit in the first rows of the gap behind the L = P + N - ctx encoded ones; a second row mask
// (mask1c) lets conv1, and nothing else, read them.  ctx = 0 is the whole-sequence path, launch for launch.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"
#include "jv_ops.h"

namespace jv {

int prompt_embed(const long* ptok, const long* plen, int P, const long* tok, const long* len, int N, const float* emb, float* rows,
                 int B, int G, int S, int vocab, hipStream_t st);
int sum_lens(const long* plen, int P, const long* len, int N, int B, long* sum, int* out32, int mul, int ctx, hipStream_t st);
int sum_lens_ctx(const long* plen, int P, const long* len, int N, int B, long* sum, int* out32, int mul, const int* ctxv,
                 int* with_ctx, hipStream_t st);
int rel_pos_table(float* pe, const float* div, int T, hipStream_t st);
int add_pos_bias(const float* qkv, const float* u, const float* v, float* qu, float* qv, long rows, hipStream_t st);
int rel_softmax(float* ac, const float* bd, const long* len, int len_mul, int B, int H, int T, int ld, int ldb, int chunk,
                hipStream_t st);
int prompt_transpose_v(const float* qkv, float* vt, int B, int T, int ld, int G, int S, hipStream_t st);
int repeat_rows2(const float* src, float* dst, int B, int T, int G, int S, int G2, int S2, hipStream_t st);
int rows_to_btc(const float* rows, const long* len, int len_mul, float* out, int B, int T, int C, int G, int S, hipStream_t st);
int lens_to_i32(const long* a, int* o, int n, int cap, hipStream_t st);   // encops.hip

constexpr int P_G = 8, P_GAP = 8;   // guard rows >= the widest context (look-ahead 3, causal 2, upsampling conv 4)
constexpr int PR_LOOKAHEAD = 3;     // pre_lookahead_len: conv1 reads rows t .. t + 3
constexpr int PR_CHUNK = 25;        // static_chunk_size of the encoder in tokens (configs: 25; x up-sampling stride 2 in stage 2)

// Sized on first use for the (B, Tk) asked for and regrown when a larger call arrives: prompts are short and rare next to
// synthesis, so this memory is not reserved at jv_create.
struct PromptWs {
  int B = 0, Tk = 0;
  bool quad = false;      // holds the three-GEMM attention's buffers (qu, qv, ac, bd, vt); the fused route needs none of them
  long* lens64 = nullptr;   // [B] p_b + n_b of the token-to-mel route
  long rows = 0;
  std::vector<void*> allocs;
  float *x = nullptr, *y = nullptr, *ln = nullptr, *qu = nullptr, *qv = nullptr, *att = nullptr;   // [rows,512]
  float* qkv = nullptr;                                                                         // [rows,1536]
  float* ffn = nullptr;                                                                         // [rows,2048]
  float* o80 = nullptr;                                                                         // [rows,80]
  float *pe = nullptr, *p = nullptr;                                                            // [2*T2,512]
  float *ac = nullptr, *bd = nullptr, *vt = nullptr;
  unsigned char *mask1 = nullptr, *mask2 = nullptr, *mask1c = nullptr;      // mask1c: mask1 + the look-ahead context rows
  int* lens_i = nullptr;
  int* lens_c = nullptr;      // [B] L_b + ctx_b of a call with per-utterance contexts: the rows mask1c marks
};

void prompt_ws_destroy(Context& c) {
  if (!c.pws) return;
  for (void* p : c.pws->allocs) (void)hipFree(p);
  delete c.pws;
  c.pws = nullptr;
}

namespace {

int ensure_ws(Context& c, int B, int Tk, bool quad) {
  if (c.pws && c.pws->B >= B && c.pws->Tk >= Tk && (c.pws->quad || !quad)) return JV_OK;
  quad = quad || (c.pws && c.pws->quad);
  const int nb = c.pws ? (B > c.pws->B ? B : c.pws->B) : B;
  const int nt = c.pws ? (Tk > c.pws->Tk ? Tk : c.pws->Tk) : Tk;
  JV_HIP(hipDeviceSynchronize());     // nothing may still be using the buffers about to be freed
  prompt_ws_destroy(c);
  PromptWs* w = new PromptWs();
  c.pws = w;
  w->B = nb; w->Tk = nt; w->quad = quad;
  const int T2 = 2 * nt;
  w->rows = round_up(P_G + nb * (T2 + P_GAP), 128) + 256;
  const size_t R = (size_t)w->rows;
  const size_t ld = (size_t)round_up(T2, 32), ldb = (size_t)round_up(2 * T2 - 1, 32);
  auto A = [&](void** p, size_t bytes) -> int {
    JV_HIP(hipMalloc(p, bytes));
    w->allocs.push_back(*p);
    JV_HIP(hipMemset(*p, 0, bytes));
    return JV_OK;
  };
  auto F = [&](float** p, size_t floats) { return A(reinterpret_cast<void**>(p), floats * sizeof(float)); };
  JV_TRY(F(&w->x, R * 512));
  JV_TRY(F(&w->y, R * 512));
  JV_TRY(F(&w->ln, R * 512));
  if (quad) JV_TRY(F(&w->qu, R * 512));
  if (quad) JV_TRY(F(&w->qv, R * 512));
  JV_TRY(F(&w->att, R * 512));
  JV_TRY(F(&w->qkv, R * 1536));
  JV_TRY(F(&w->ffn, R * 2048));
  JV_TRY(F(&w->o80, R * 80));
  JV_TRY(F(&w->pe, (size_t)ldb * 512));
  JV_TRY(F(&w->p, (size_t)(ldb + 128) * 512));
  if (quad) JV_TRY(F(&w->ac, (size_t)nb * 8 * T2 * ld));
  if (quad) JV_TRY(F(&w->bd, (size_t)nb * 8 * T2 * ldb));
  if (quad) JV_TRY(F(&w->vt, (size_t)nb * 8 * 64 * ld));
  JV_TRY(A(reinterpret_cast<void**>(&w->lens64), sizeof(long) * nb));
  JV_TRY(A(reinterpret_cast<void**>(&w->mask1), R));
  JV_TRY(A(reinterpret_cast<void**>(&w->mask2), R));
  JV_TRY(A(reinterpret_cast<void**>(&w->mask1c), R));
  JV_TRY(A(reinterpret_cast<void**>(&w->lens_i), sizeof(int) * nb));
  JV_TRY(A(reinterpret_cast<void**>(&w->lens_c), sizeof(int) * nb));
  return JV_OK;
}

ConvGemmArgs lin_args(const float* A, int lda, long a_rows, long M, const GemmW& w, float* out, int ldo) {
  ConvGemmArgs a;
  conv_gemm_defaults(a);
  a.A = A; a.lda = lda; a.a_rows = a_rows; a.M = (int)M;
  a.Cin = w.Cin; a.ntaps = w.ntaps; a.tap_row0 = 0; a.tap_dil = 1;
  a.W = w.w; a.ldw = w.ldw; a.n_rows_w = w.n_rows; a.N = w.N; a.bias = w.bias;
  a.W3 = w.w3; a.w3_plane = (long)w.n_rows * w.ldw;
  a.out = out; a.ldo = ldo;
  return a;
}

}  // namespace

// The block's attention as three batched GEMMs around the rel-shift softmax, on explicit buffers (the conformer block's own
// workspace, or jv_op_rel_attention's): qu, qv [rows, 512]; ac [B,8,T,ld], bd [B,8,T,ldb], vt [B,8,64,ld], ld = round_up(T, 32),
// ldb = round_up(2T - 1, 32); p must be readable for round_up(2T - 1, 64) rows (the GEMM's weight-tile loads).
int rel_attention_gemm(const float* qkv, const float* p, const float* u, const float* v, float* qu, float* qv, float* ac, float* bd,
                       float* vt, float* att, const long* len, int len_mul, int B, int T, int G, int S, int chunk, hipStream_t st) {
  const int ld = round_up(T, 32), npos = 2 * T - 1, ldb = round_up(npos, 32);
  const long M = (long)G + (long)B * S;
  ConvGemmArgs a;
  JV_TRY(add_pos_bias(qkv, u, v, qu, qv, M, st));
  // ac[b,h] = (q + u) K^T : the K rows are the K-contiguous "weight" operand
  conv_gemm_defaults(a);
  a.A = qu + (long)G * 512; a.lda = 512; a.a_rows = T; a.M = T; a.Cin = 64; a.ntaps = 1;
  a.W = qkv + (long)G * 1536 + 512; a.ldw = 1536; a.n_rows_w = T; a.N = T;
  a.out = ac; a.ldo = ld;
  a.nb2 = 8;
  a.sA1 = (long)S * 512; a.sA2 = 64; a.sW1 = (long)S * 1536; a.sW2 = 64; a.sO1 = 8L * T * ld; a.sO2 = (long)T * ld;
  JV_TRY(conv_gemm(a, B * 8, st));
  // bd[b,h] = (q + v) P_h^T over all 2T-1 relative positions (rel_shift happens inside the softmax's indexing)
  conv_gemm_defaults(a);
  a.A = qv + (long)G * 512; a.lda = 512; a.a_rows = T; a.M = T; a.Cin = 64; a.ntaps = 1;
  a.W = p; a.ldw = 512; a.n_rows_w = npos; a.N = npos;
  a.out = bd; a.ldo = ldb;
  a.nb2 = 8;
  a.sA1 = (long)S * 512; a.sA2 = 64; a.sW1 = 0; a.sW2 = 64; a.sO1 = 8L * T * ldb; a.sO2 = (long)T * ldb;
  JV_TRY(conv_gemm(a, B * 8, st));
  JV_TRY(rel_softmax(ac, bd, len, len_mul, B, 8, T, ld, ldb, chunk, st));
  JV_TRY(prompt_transpose_v(qkv, vt, B, T, ld, G, S, st));
  // att[b, :, h*64:(h+1)*64] = P_bh V_bh
  conv_gemm_defaults(a);
  a.A = ac; a.lda = ld; a.a_rows = T; a.M = T; a.Cin = ld; a.ntaps = 1;
  a.W = vt; a.ldw = ld; a.n_rows_w = 64; a.N = 64;
  a.out = att + (long)G * 512; a.ldo = 512;
  a.nb2 = 8;
  a.sA1 = 8L * T * ld; a.sA2 = (long)T * ld; a.sW1 = 8L * 64 * ld; a.sW2 = 64L * ld; a.sO1 = (long)S * 512; a.sO2 = 64;
  return conv_gemm(a, B * 8, st);
}

namespace {

// jv_upsample_encoder_tap: the stage whose buffer encoder_stages copies out before it returns early (null: the whole encoder)
struct UpsTap {
  int id;
  float* out;
  long out_floats;
};

struct UpsTapShape {
  int C;        // channels of a row tap
  int rate;     // 1: token rows, 2: mel rows
  bool table;   // [2T - 1, 512], no batch geometry (the position tables and linear_pos of them)
};

// false: no such tap
bool ups_tap_shape(int id, UpsTapShape& s) {
  if (id < 0 || id >= JV_UPS_TAP_COUNT) return false;
  s.C = 512;
  s.rate = id >= JV_UPS_TAP_REP ? 2 : 1;
  s.table = id == JV_UPS_TAP_PE1 || id == JV_UPS_TAP_PE2;
  if (id == JV_UPS_TAP_H) s.C = 80;
  int kind = -1;
  if (id >= JV_UPS_TAP_LN1_0 && id < JV_UPS_TAP_REP) kind = (id - JV_UPS_TAP_LN1_0) % JV_UPS_TAP_PER_BLOCK;
  if (id >= JV_UPS_TAP_ULN1_0 && id < JV_UPS_TAP_AN) kind = (id - JV_UPS_TAP_ULN1_0) % JV_UPS_TAP_PER_BLOCK;
  if (kind == JV_UPS_TAP_QKV_0 - JV_UPS_TAP_LN1_0) s.C = 1536;
  if (kind == JV_UPS_TAP_FF_0 - JV_UPS_TAP_LN1_0) s.C = 2048;
  if (kind == JV_UPS_TAP_POS_0 - JV_UPS_TAP_LN1_0) s.table = true;
  return true;
}

// ahead of an entry's first launch.  W: tokens of the whole sequence (P + N), Tenc: the encoded width (W less a scalar context)
int check_tap(const UpsTap* tap, int B, int W, int Tenc) {
  if (!tap) return JV_OK;
  UpsTapShape s;
  if (!ups_tap_shape(tap->id, s)) return fail(JV_ERR_ARG, "jv_upsample_encoder_tap: unknown tap");
  const long need = s.table ? (2L * s.rate * Tenc - 1) * 512 : (long)B * s.C * s.rate * W;
  if (tap->out_floats < need)
    return fail(JV_ERR_SHAPE, "jv_upsample_encoder_tap: out holds fewer floats than the tap ([B, C, rate (P + N)], a table [2T - 1, 512])");
  return JV_OK;
}

// one pre-LN block on T rows per utterance (geometry G, S): x += MHA_rel(LN(x)); x += W2 silu(W1 LN(x)).  fused: the attention
// as relattn.hip's one launch instead of the three GEMMs; chunk > 0: the streaming mask (keys j < (i / chunk + 1) * chunk)
// tap_kind (jv_upsample_encoder_tap; -1: none): return behind the launches of that one of the block's eight stages, *tap_buf = the
// buffer it stands in (x is updated in place: a stage can only be read where it stands)
int conformer_block(Context& c, const ConfBlockW& k, int B, int T, int G, int S, long M, const long* len, int len_mul, bool fused,
                    int chunk, hipStream_t st, int tap_kind = -1, const float** tap_buf = nullptr) {
  PromptWs& w = *c.pws;
  const long AR = w.rows;
  const int npos = 2 * T - 1;
  auto at = [&](int id, const float* buf) {
    if (tap_kind != id - JV_UPS_TAP_LN1_0) return false;
    *tap_buf = buf;
    return true;
  };
  JV_TRY(layernorm_rows(w.x, nullptr, w.ln, k.n_mha.g, k.n_mha.b, 1e-5f, M, 512, nullptr, st));
  if (at(JV_UPS_TAP_LN1_0, w.ln)) return JV_OK;
  ConvGemmArgs a = lin_args(w.ln, 512, AR, M, k.qkv, w.qkv, 1536);
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_QKV_0, w.qkv)) return JV_OK;
  a = lin_args(w.pe, 512, npos, npos, k.pos, w.p, 512);                       // p = linear_pos(pos_emb), shared by the batch
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_POS_0, w.p)) return JV_OK;
  if (fused) JV_TRY(rel_attention(w.qkv, w.p, npos, k.u, k.v, len, len_mul, B, T, G, S, chunk, w.att, st));
  else JV_TRY(rel_attention_gemm(w.qkv, w.p, k.u, k.v, w.qu, w.qv, w.ac, w.bd, w.vt, w.att, len, len_mul, B, T, G, S, chunk, st));
  if (at(JV_UPS_TAP_ATT_0, w.att)) return JV_OK;
  a = lin_args(w.att, 512, AR, M, k.out, w.x, 512);
  a.res1 = w.x; a.ldr1 = 512;
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_X1_0, w.x)) return JV_OK;
  JV_TRY(layernorm_rows(w.x, nullptr, w.ln, k.n_ff.g, k.n_ff.b, 1e-5f, M, 512, nullptr, st));
  if (at(JV_UPS_TAP_LN2_0, w.ln)) return JV_OK;
  a = lin_args(w.ln, 512, AR, M, k.w1, w.ffn, 2048);
  a.act = ACT_SILU;
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_FF_0, w.ffn)) return JV_OK;
  a = lin_args(w.ffn, 2048, AR, M, k.w2, w.x, 512);
  a.res1 = w.x; a.ldr1 = 512;
  JV_TRY(conv_gemm(a, 1, st));
  (void)at(JV_UPS_TAP_X2_0, w.x);
  return JV_OK;
}

// Both stages for utterance b's ids [ptok[b, :p_b] | tok[b, :n_b]] (P = 0: one source), T1 = P + N token rows.  `len`: the int64
// lengths p_b + n_b - ctx on the device.  fused / streaming: the attention route and the chunk masks of conformer_block.
// ctx > 0 (< P_GAP): the last ctx tokens of the P + N are context of the look-ahead convolution only; every length below is the
// encoded one, T1 = P + N - ctx
// lens_c (with ctx = 0): every utterance has a context of its own, 0 or 3 tokens.  The buffers keep the width of the whole
// sequence, T1 = P + N; utterance b's context rows sit right behind its L_b = len[b] encoded ones -- rows that are padding to
// everything but conv1 -- and lens_c[b] = L_b + ctx_b is what mask1c marks
// tap (jv_upsample_encoder_tap, else null): return behind the launches of that stage, its buffer copied out (the entry has checked
// the tap and the size of its `out`); nothing ahead of the return depends on it, and h_out is not written
int encoder_stages(Context& c, const long* ptok, const long* plen, int P, const long* tok, const long* tlen, int N, const long* len,
                   int B, bool fused, bool streaming, int ctx, float* h_out, hipStream_t st, const int* lens_c = nullptr,
                   const UpsTap* tap = nullptr) {
  PromptWs& w = *c.pws;
  const PromptW& e = c.prompt;
  const long AR = w.rows;
  const int Tk = P + N - ctx;
  const int T1 = Tk, S1 = T1 + P_GAP, T2 = 2 * Tk, S2 = T2 + P_GAP;
  const long M1 = P_G + (long)B * S1, M2 = P_G + (long)B * S2;
  const int chunk1 = streaming ? PR_CHUNK : 0, chunk2 = 2 * chunk1;
  auto at = [&](int id) { return tap && tap->id == id; };
  // row taps: [B, C, rate (P + N)] channels first, zeros at and behind rate * lens[b] + add (lens_i holds the encoded lengths L_b)
  auto tap_rows = [&](const float* buf, const int* lens, int add) -> int {
    UpsTapShape s;
    ups_tap_shape(tap->id, s);
    const int Wd = s.rate * (P + N);
    return rows_to_cf(buf, s.C, 0, P_G, s.rate == 1 ? S1 : S2, tap->out, (long)s.C * Wd, B, s.C, Wd, lens, st, nullptr, s.rate, add);
  };
  auto tap_table = [&](const float* buf, int T) -> int {
    JV_HIP(hipMemcpyAsync(tap->out, buf, sizeof(float) * (2L * T - 1) * 512, hipMemcpyDeviceToDevice, st));
    return JV_OK;
  };
  // the eight taps of block i of a stage whose block 0 starts at id0: which of them the block stops behind (-1: none)
  auto block_tap = [&](int id0, int i) {
    const int k = tap ? tap->id - (id0 + JV_UPS_TAP_PER_BLOCK * i) : -1;
    return k >= 0 && k < JV_UPS_TAP_PER_BLOCK ? k : -1;
  };
  auto block_out = [&](int kind, const float* buf, int T) -> int {
    return kind == JV_UPS_TAP_POS_0 - JV_UPS_TAP_LN1_0 ? tap_table(buf, T) : tap_rows(buf, w.lens_i, 0);
  };

  JV_TRY(lens_to_i32(len, w.lens_i, B, Tk, st));
  JV_TRY(row_meta(w.mask1, nullptr, w.lens_i, B, 1, P_G, S1, T1, AR, 1, 0, st));
  JV_TRY(row_meta(w.mask2, nullptr, w.lens_i, B, 1, P_G, S2, T2, AR, 2, 0, st));
  if (ctx > 0) JV_TRY(row_meta(w.mask1c, nullptr, w.lens_i, B, 1, P_G, S1, T1 + ctx, AR, 1, ctx, st));      // rows [0, len + ctx)
  if (lens_c) JV_TRY(row_meta(w.mask1c, nullptr, lens_c, B, 1, P_G, S1, T1, AR, 1, 0, st));                 // rows [0, len_b + ctx_b)

  // ---- stage 1: embedding -> Linear + LayerNorm (* sqrt 512) -> look-ahead convs -> 6 blocks ---------------------------
  JV_TRY(fill(w.y, 0.f, M1 * 512, st));                     // gap rows of the embedding buffer must read as zero tokens
  JV_TRY(prompt_embed(ptok, plen, P, tok, tlen, N, e.emb, w.y, B, P_G, S1, PR_VOCAB, st));
  if (at(JV_UPS_TAP_EMB)) return tap_rows(w.y, w.lens_i, 0);
  ConvGemmArgs a = lin_args(w.y, 512, AR, M1, e.emb_lin, w.ln, 512);
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_EL)) return tap_rows(w.ln, w.lens_i, 0);
  JV_TRY(layernorm_rows(w.ln, nullptr, w.x, e.emb_ln.g, e.emb_ln.b, 1e-5f, M1, 512, nullptr, st));
  if (at(JV_UPS_TAP_E0)) return lens_c ? tap_rows(w.x, lens_c, 0) : tap_rows(w.x, w.lens_i, ctx);      // the rows conv1 reads
  JV_TRY(rel_pos_table(w.pe, e.div, T1, st));
  if (at(JV_UPS_TAP_PE1)) return tap_table(w.pe, T1);
  // conv1: rows t .. t+3 of the valid frames (zeros beyond the end -- or, behind the last encoded frame of a partial sequence, the
  // embedded context rows), bias; LeakyReLU(0.01) is conv2's prologue
  a = lin_args(w.x, 512, AR, M1, e.look1, w.y, 512);
  a.tap_row0 = 0;
  a.rowmask_in = ctx > 0 || lens_c ? w.mask1c : w.mask1;
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_C1)) return tap_rows(w.y, w.lens_i, 0);
  // conv2: rows t-2 .. t of leaky(conv1) over the valid frames (zeros before the start), + bias + x
  a = lin_args(w.y, 512, AR, M1, e.look2, w.ln, 512);
  a.tap_row0 = -2;
  a.rowmask_in = w.mask1;
  a.pro = PRO_LRELU; a.pro_slope = 0.01f;
  a.res1 = w.x; a.ldr1 = 512;
  JV_TRY(conv_gemm(a, 1, st));
  JV_HIP(hipMemcpyAsync(w.x, w.ln, sizeof(float) * M1 * 512, hipMemcpyDeviceToDevice, st));
  if (at(JV_UPS_TAP_LA)) return tap_rows(w.x, w.lens_i, 0);
  for (int i = 0; i < PR_BLOCKS; ++i) {
    const int kind = block_tap(JV_UPS_TAP_LN1_0, i);
    const float* buf = nullptr;
    JV_TRY(conformer_block(c, e.blk[i], B, T1, P_G, S1, M1, len, 1, fused, chunk1, st, kind, &buf));
    if (kind >= 0) return block_out(kind, buf, T1);
  }

  // ---- stage 2: nearest x2 -> conv k5 over rows u-4 .. u -> Linear + LayerNorm (* sqrt 512) -> 4 blocks -> LN -> proj ----
  JV_TRY(fill(w.y, 0.f, M2 * 512, st));
  JV_TRY(repeat_rows2(w.x, w.y, B, T1, P_G, S1, P_G, S2, st));
  if (at(JV_UPS_TAP_REP)) return tap_rows(w.y, w.lens_i, 0);
  a = lin_args(w.y, 512, AR, M2, e.up_conv, w.ln, 512);
  a.tap_row0 = -4;
  a.rowmask_in = w.mask2;
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_UP)) return tap_rows(w.ln, w.lens_i, 0);
  a = lin_args(w.ln, 512, AR, M2, e.up_emb_lin, w.y, 512);
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_UL)) return tap_rows(w.y, w.lens_i, 0);
  JV_TRY(layernorm_rows(w.y, nullptr, w.x, e.up_emb_ln.g, e.up_emb_ln.b, 1e-5f, M2, 512, nullptr, st));
  if (at(JV_UPS_TAP_U0)) return tap_rows(w.x, w.lens_i, 0);
  JV_TRY(rel_pos_table(w.pe, e.div, T2, st));
  if (at(JV_UPS_TAP_PE2)) return tap_table(w.pe, T2);
  for (int i = 0; i < PR_UP_BLOCKS; ++i) {
    const int kind = block_tap(JV_UPS_TAP_ULN1_0, i);
    const float* buf = nullptr;
    JV_TRY(conformer_block(c, e.up[i], B, T2, P_G, S2, M2, len, 2, fused, chunk2, st, kind, &buf));
    if (kind >= 0) return block_out(kind, buf, T2);
  }
  JV_TRY(layernorm_rows(w.x, nullptr, w.ln, e.after.g, e.after.b, 1e-5f, M2, 512, nullptr, st));
  if (at(JV_UPS_TAP_AN)) return tap_rows(w.ln, w.lens_i, 0);
  a = lin_args(w.ln, 512, AR, M2, e.proj, w.o80, 80);
  JV_TRY(conv_gemm(a, 1, st));
  if (at(JV_UPS_TAP_H)) return tap_rows(w.o80, w.lens_i, 0);
  return rows_to_btc(w.o80, len, 2, h_out, B, T2, 80, P_G, S2, st);
}

int check_encoder_call(Context& c, int B, int Tk) {
  if (!c.ready[MODEL_PROMPT]) return fail(JV_ERR_STATE, "prompt encoder weights not finalized");
  if (B < 1 || Tk < 1) return fail(JV_ERR_ARG, "batch and token count must be positive");
  if (B > c.max_batch || 2 * Tk > c.max_frames || Tk > 2048)
    return fail(JV_ERR_SHAPE, "prompt batch/tokens exceed the capacity given to jv_create (2*tokens <= max_frames, tokens <= 2048)");
  return JV_OK;
}

// The three entries, each with the optional tap of jv_upsample_encoder_tap (checked behind the entry's own checks, ahead of its
// first launch); the functions the rest of the library calls pass none
int prompt_encoder_run(Context& c, const long* tok, const long* len, int B, int Tk, float* h_out, hipStream_t st, const UpsTap* tap) {
  JV_TRY(check_encoder_call(c, B, Tk));
  JV_TRY(check_tap(tap, B, Tk, Tk));
  JV_TRY(ensure_ws(c, B, Tk, true));
  // the three-GEMM attention, full context: this entry's launches and bits are what they were before relattn.hip existed
  return encoder_stages(c, nullptr, nullptr, 0, tok, len, Tk, len, B, false, false, 0, h_out, st, nullptr, tap);
}

// flow.py:319-328, 338: [prompt tokens | tokens] -> h, on the fused attention (no ac / bd / vt in this route's workspace)
// ctx = 3: flow.py:330-336, h over the first P + N - 3 tokens with the last three as look-ahead context ([B, 2 (P + N - 3), 80])
int flow_encoder_run(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, int B, int P, int N,
                     int streaming, float* h_out, int* h_lens, hipStream_t st, int ctx, const UpsTap* tap) {
  if (P < 0 || N < 0) return fail(JV_ERR_ARG, "jv_flow_encoder_fwd: P and N must be non-negative");
  if (ctx != 0 && ctx != PR_LOOKAHEAD) return fail(JV_ERR_ARG, "flow encoder: the context is the look-ahead length (3 tokens) or nothing");
  if (ctx > 0 && (B != 1 || P + N <= ctx)) return fail(JV_ERR_ARG, "partial flow encoder: B must be 1 and P + N at least 4 (one encoded token + 3 of context)");
  JV_TRY(check_encoder_call(c, B, P + N));
  JV_TRY(check_tap(tap, B, P + N, P + N - ctx));
  JV_TRY(ensure_ws(c, B, P + N, false));
  PromptWs& w = *c.pws;
  JV_TRY(sum_lens(plen, P, len, N, B, w.lens64, h_lens, 2, ctx, st));
  return encoder_stages(c, ptok, plen, P, tok, len, N, w.lens64, B, true, streaming != 0, ctx, h_out, st, nullptr, tap);
}

}  // namespace

int prompt_encoder_fwd(Context& c, const long* tok, const long* len, int B, int Tk, float* h_out, hipStream_t st) {
  return prompt_encoder_run(c, tok, len, B, Tk, h_out, st, nullptr);
}

int flow_encoder_fwd(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, int B, int P, int N,
                     int streaming, float* h_out, int* h_lens, hipStream_t st, int ctx) {
  return flow_encoder_run(c, ptok, plen, tok, len, B, P, N, streaming, h_out, h_lens, st, ctx, nullptr);
}

// The lengths of a call with per-utterance contexts, on the host: the token counts and ctx_lens come down (one synchronisation, the
// call's only one) and are checked before anything is launched on them.  enc_lens[b] receives L_b = m_b - ctx_b.  A wrong context
// is a wrong sequence end, which a clamp would turn into other frames silently: rejected, naming the utterance.
int flow_ctx_lengths(const char* who, const long* plen, const long* len, const int* ctx_lens, const int* extra, int B, int P, int N,
                     std::vector<int>& enc_lens, std::vector<int>* extra_host, hipStream_t st) {
  if (B < 1 || P < 0 || N < 0) return fail(JV_ERR_ARG, std::string(who) + ": B must be positive, P and N non-negative");
  std::vector<long> pl(B, 0), tl(B, 0);
  std::vector<int> cx(B, 0);
  if (P > 0) JV_HIP(hipMemcpyAsync(pl.data(), plen, sizeof(long) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipMemcpyAsync(tl.data(), len, sizeof(long) * B, hipMemcpyDeviceToHost, st));
  JV_HIP(hipMemcpyAsync(cx.data(), ctx_lens, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  if (extra && extra_host) {
    extra_host->assign(B, 0);
    JV_HIP(hipMemcpyAsync(extra_host->data(), extra, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  }
  JV_HIP(hipStreamSynchronize(st));
  enc_lens.assign(B, 0);
  for (int b = 0; b < B; ++b) {
    const long m = std::min(std::max(pl[b], 0L), (long)P) + std::min(std::max(tl[b], 0L), (long)N);
    char msg[200];
    if (cx[b] != 0 && cx[b] != PR_LOOKAHEAD) {
      snprintf(msg, sizeof msg, "%s: utterance %d: context %d: the look-ahead length (3 tokens) or nothing", who, b, cx[b]);
      return fail(JV_ERR_ARG, msg);
    }
    if (m - cx[b] < 1) {
      snprintf(msg, sizeof msg, "%s: utterance %d: %ld tokens with a context of %d: at least one encoded token is needed", who, b, m,
               cx[b]);
      return fail(JV_ERR_ARG, msg);
    }
    enc_lens[b] = (int)(m - cx[b]);
  }
  return JV_OK;
}

// jv_flow_encoder_fwd_ctx: flow_encoder_fwd with a context per utterance (ctx_lens: device int32 [B], each 0 or 3), h [B, 2 (P + N), 80]
// with zeros behind 2 L_b.  checked: the caller has run flow_ctx_lengths on these vectors already
static int flow_encoder_ctx_run(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, const int* ctx_lens,
                                int B, int P, int N, int streaming, float* h_out, int* h_lens, hipStream_t st, bool checked,
                                const UpsTap* tap) {
  if (P < 0 || N < 0) return fail(JV_ERR_ARG, "jv_flow_encoder_fwd_ctx: P and N must be non-negative");
  JV_TRY(check_encoder_call(c, B, P + N));
  if (!checked) {
    std::vector<int> enc_lens;
    JV_TRY(flow_ctx_lengths("jv_flow_encoder_fwd_ctx", plen, len, ctx_lens, nullptr, B, P, N, enc_lens, nullptr, st));
  }
  JV_TRY(check_tap(tap, B, P + N, P + N));
  JV_TRY(ensure_ws(c, B, P + N, false));
  PromptWs& w = *c.pws;
  JV_TRY(sum_lens_ctx(plen, P, len, N, B, w.lens64, h_lens, 2, ctx_lens, w.lens_c, st));
  return encoder_stages(c, ptok, plen, P, tok, len, N, w.lens64, B, true, streaming != 0, 0, h_out, st, w.lens_c, tap);
}

int flow_encoder_fwd_ctx(Context& c, const long* ptok, const long* plen, const long* tok, const long* len, const int* ctx_lens, int B,
                         int P, int N, int streaming, float* h_out, int* h_lens, hipStream_t st, bool checked) {
  return flow_encoder_ctx_run(c, ptok, plen, tok, len, ctx_lens, B, P, N, streaming, h_out, h_lens, st, checked, nullptr);
}

// jv_upsample_encoder_tap: one of the entries above with a tap
int upsample_encoder_tap(Context& c, int mode, const long* ptok, const long* plen, const long* tok, const long* len, const int* ctx_lens,
                         int B, int P, int N, int streaming, int tap_id, float* out, long out_floats, hipStream_t st) {
  const UpsTap tap{tap_id, out, out_floats};
  switch (mode) {
    case JV_UPS_MODE_PROMPT:
      if (P != 0 || streaming != 0) return fail(JV_ERR_ARG, "jv_upsample_encoder_tap: the prompt entry has no prompt tokens (P = 0) and no streaming");
      return prompt_encoder_run(c, tok, len, B, N, nullptr, st, &tap);
    case JV_UPS_MODE_FLOW:
      return flow_encoder_run(c, ptok, plen, tok, len, B, P, N, streaming, nullptr, nullptr, st, 0, &tap);
    case JV_UPS_MODE_PARTIAL:
      if (B != 1) return fail(JV_ERR_ARG, "jv_upsample_encoder_tap: the partial entry is B = 1");
      return flow_encoder_run(c, ptok, plen, tok, len, 1, P, N, streaming, nullptr, nullptr, st, PR_LOOKAHEAD, &tap);
    case JV_UPS_MODE_CTX:
      if (!ctx_lens) return fail(JV_ERR_ARG, "jv_upsample_encoder_tap: the per-utterance mode needs ctx_lens");
      return flow_encoder_ctx_run(c, ptok, plen, tok, len, ctx_lens, B, P, N, streaming, nullptr, nullptr, st, false, &tap);
  }
  return fail(JV_ERR_ARG, "jv_upsample_encoder_tap: mode is JV_UPS_MODE_PROMPT, _FLOW, _PARTIAL or _CTX");
}

}  // namespace jv

extern "C" {

int jv_prompt_encoder_fwd(jv_context* ctx, const int64_t* tokens, const int64_t* token_len, int B, int Tk, float* prompt_h,
                          void* stream) {
  if (!ctx || !tokens || !token_len || !prompt_h) return jv::fail(JV_ERR_ARG, "jv_prompt_encoder_fwd: null argument");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::prompt_encoder_fwd(ctx->c, reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_len), B, Tk,
                                prompt_h, static_cast<hipStream_t>(stream));
}

int jv_flow_encoder_fwd(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                        const int64_t* token_lens, int B, int P, int N, int streaming, float* h, int32_t* h_lens, void* stream) {
  if (!ctx || !h || !token_lens || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)))
    return jv::fail(JV_ERR_ARG, "jv_flow_encoder_fwd: null argument");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::flow_encoder_fwd(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                              reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), B, P, N, streaming, h,
                              h_lens, static_cast<hipStream_t>(stream));
}

int jv_flow_encoder_fwd_ctx(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                            const int64_t* token_lens, const int32_t* ctx_lens, int B, int P, int N, int streaming, float* h,
                            int32_t* h_lens, void* stream) {
  if (!ctx || !h || !token_lens || !ctx_lens || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)))
    return jv::fail(JV_ERR_ARG, "jv_flow_encoder_fwd_ctx: null argument");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::flow_encoder_fwd_ctx(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                                  reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), ctx_lens, B, P, N,
                                  streaming, h, h_lens, static_cast<hipStream_t>(stream), false);
}

int jv_upsample_encoder_tap(jv_context* ctx, int mode, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                            const int64_t* token_lens, const int32_t* ctx_lens, int B, int P, int N, int streaming, int tap,
                            float* out, int64_t out_floats, void* stream) {
  if (!ctx || !out || !token_lens || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)))
    return jv::fail(JV_ERR_ARG, "jv_upsample_encoder_tap: null argument");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::upsample_encoder_tap(ctx->c, mode, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                                  reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), ctx_lens, B, P, N,
                                  streaming, tap, out, (long)out_floats, static_cast<hipStream_t>(stream));
}

int jv_flow_encoder_fwd_partial(jv_context* ctx, const int64_t* prompt_tokens, const int64_t* prompt_lens, const int64_t* tokens,
                                const int64_t* token_lens, int P, int N, int streaming, float* h, int32_t* h_lens, void* stream) {
  if (!ctx || !h || !token_lens || (N > 0 && !tokens) || (P > 0 && (!prompt_tokens || !prompt_lens)))
    return jv::fail(JV_ERR_ARG, "jv_flow_encoder_fwd_partial: null argument");
  JV_HIP(hipSetDevice(ctx->c.device));
  return jv::flow_encoder_fwd(ctx->c, reinterpret_cast<const long*>(prompt_tokens), reinterpret_cast<const long*>(prompt_lens),
                              reinterpret_cast<const long*>(tokens), reinterpret_cast<const long*>(token_lens), 1, P, N, streaming, h,
                              h_lens, static_cast<hipStream_t>(stream), jv::PR_LOOKAHEAD);
}

}  // extern "C"
