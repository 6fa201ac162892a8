// Flow-matching decoder: one estimator evaluation (jyutvoice/flow/decoder.py:917-1018).  Everything runs on row buffers [G + b*S + t][C] (jv_common.h): the estimator's `b c t <-> b t c`
// transposes (decoder.py:950,966) disappear, causal convolutions are 3-tap row-offset GEMMs, and the
// 2B CFG rows are just more rows.  Per estimator call: 3 tiny time-MLP GEMMs, 14 x (3 conv GEMMs) +
// 56 x (2 LayerNorm + 4 GEMM + 1 attention) + 4 tail launches -- fewer wherever the route (est_route) fuses them -- all
// enqueued on the caller's stream with no host synchronisation (graph-capturable).
// est_route() decides every regime of a call once; Est launches what the record says and tests no switch itself.
#include <stdio.h>

#include <algorithm>

#include "../../include/jyutvoice_hip.h"
#include "flow_ws.h"

namespace jv {

// The route of a call over M rows.  `temb_pre`: the step's time embedding is precomputed (cfm_solve); `compact`: the rows are
// laid out compactly; `res_one` = false: the caller rules the whole-resnet launch out; the mode switches, the tile height and the
// load-time weight bits are read here and nowhere else.
EstRoute est_route(const Context& c, long M, bool temb_pre, bool compact, int attn_chunk, bool res_one) {
  const EstimatorW& e = c.est;
  EstRoute r;
  const int tile = rowgemm_tile((int)M);
  r.exact = c.exact_range; r.compact = compact; r.attn_chunk = attn_chunk;
  // FP16 mode (jv_flow_set_precision; never together with exact_range): one product per fp16x3 step, and every plane-fed
  // attention on attn64_pl -- attn64_s has no one-product slot sequence (DESIGN.md 5 "FP16 mode")
  r.np = c.est_fp16 && !c.exact_range ? 1 : 3;
  r.attn_single = r.np == 3;
  // the row-owning kernels (rowgemm_kernel.h, rowconv_kernel.h: LayerNorm / Mish / mask / time embedding / residual in the
  // epilogue, no stand-alone row-wise pass) when the batch fills the chip, else the tile kernels
  r.rows = !c.exact_range && !c.no_rowgemm && tile > 0;
  // ---- short M (a single utterance: 268 rows = 20 tiles of 64x64): the K = 512 ... 1536 contractions to 256 channels are
  // split over ksplit workgroups per tile (ConvGemmArgs::ksplit) and one row-wise kernel sums the partials and runs the
  // whole tail -- bias, LayerNorm / Mish / mask, time embedding, residual, tracking, and the LayerNorm that feeds the next
  // GEMM (splitk_reduce_rows).  Traced at B = 1: ff.net.2 + its LayerNorm 20.8 + 4.8 us -> 2 x ~5.
  // The split is a function of K alone (PARTIAL_SPLITS shares of the chunks whenever M <= PARTIAL_ROWS), never of M: the
  // grouping of a row's partial sums must not depend on how many rows the batch has, or a shard would no longer reproduce
  // the whole batch bit for bit (tests/test_gpu_dist.py).
  // ... and never together with the row-owning kernels (the debugging override JV_ROWGEMM_RT can force those at short M):
  // the split-K tails hand the next LayerNorm on as fp32 rows, the row-owning blocks read fp16 planes from the same buffer
  // Split-K lives in the split-plane kernels (conv_gemm_x6); a launch that would take the fp32-MFMA route (no weight
  // planes, unaligned ldw, JV_NO_X6) runs unsplit instead
  r.ksplit = (M <= PARTIAL_ROWS && tile == 0 && !dyn_env("JV_NO_X6")) ? PARTIAL_SPLITS : 1;
  // one decision for every block of the call (a block's split-K tail writes the NEXT block's LayerNorm): all of them take
  // the split-plane route, or none is split
  r.sk_blocks = r.ksplit > 1 && !c.dma_a && e.sk_ok;
  r.pre_planes = c.dma_a && !c.exact_range;
  r.ffn_fuse = !c.no_ffn_fuse;
  r.block_fuse = !c.no_block_fuse && r.ffn_fuse;
  // Few row tiles (3 - 10 utterances of 300 frames: 64 - 192 workgroups of 32 rows on 256 CUs): a workgroup's length is set
  // by the weights it streams through its CU's L2 port, not by its MFMAs, and a third of the fused block's steps are the
  // next block's q | k | v, whose six 256-column chunks need nothing from each other.  There the q | k | v phase leaves the
  // fused launch: phase B's epilogue writes the LayerNorm1 planes to HBM and rowgemm_wa runs with its chunks dealt over
  // qkv_split workgroups per row tile.  Same K order, same epilogue expressions: the same bits as the fused launch
  // (tests/test_gpu_pipeline.py::test_split_qkv_equals_fused_block).  JV_NO_QKV_SPLIT=1: fused at every batch size.
  // The stand-alone launch takes the TALLEST tile: what a launch requests from L2 is (row tiles) x (weight bytes) -- at 152
  // tiles of 32 rows 228 MB, and dealing the chunks of those tiles out moved it only from 27 to 21 us -- so 80-row tiles (61
  // of them at 8 utterances, 92 MB) with as many column groups as fit one round of the chip: 19 us.
  if (r.rows && !c.no_qkv_split && cdivl(M, 16 * tile) <= 192) {
    r.qkv_rt = 5;
    const long tiles = cdivl(M, 80);
    r.qkv_split = tiles * 6 <= 256 ? 6 : tiles * 3 <= 256 ? 3 : 2;
  }
  // may a ragged batch of M rows take the compact geometry?  Only the route whose every kernel knows it: the row-owning
  // kernels with the plane attention, in every stage
  r.compact_ok = !c.no_compact && r.rows && e.rows_ok && attn_chunk == 0;

  // (the row-owning convolution streams this weight straight into registers)
  auto w_direct = [](const GemmW& m) { RowConvArgs a{}; a.Wf = m.wf; a.Cin = m.Cin; return rowconv_w_direct(a); };
  auto planes = [](const GemmW& m) { return (m.w3 || m.w2) && !(m.ldw & 7); };
  // The whole resnet in ONE launch (rowres_kernel.h) where every piece has its row-owning form: a trunk input with a
  // measured bound (not the first resnet's), fragment-order weights for block1 | res_conv and for block2, the step's time
  // embedding shared by all rows (cfm_solve), a tile height that keeps the launch in as many rounds as the two it replaces.
  // JV_NO_RES_PAIR=1: two.
  const bool one = res_one && r.rows && !c.no_res_pair && !c.no_res_fold && temb_pre && rowres_fits((int)M);
  // A workgroup reads its neighbours' rows as halo, so the launch never writes the buffer it reads: the mid stages alternate the
  // trunk between w.h and w.h2 (free: the launch keeps block1's output in LDS).  Decided for the trunk as a whole -- an even
  // number of stages, ALL paired, brings it back to w.h; one resnet that cannot (an unusable h2_bound) would run its two
  // launches in place wherever its predecessors left the trunk, and block1's output buffer is w.h2.
  const bool mid_one = one && EST_NMID % 2 == 0 && e.mid_pair_ok;
  for (int i = 0; i < EST_NRES; ++i) {
    EstRoute::Stage& s = r.stage[i];
    const ResnetW& rn = e.res[i];
    s.rows = r.rows && e.stage_rows_ok[i];
    s.res = (i >= 1 && i <= EST_NMID ? mid_one : one && i > 0 && rn.pair_ok) ? RES_ONE : r.rows ? RES_ROWS : RES_TILES;
    // (the first resnet reads xin, which has no tracked bound: its block1 and res_conv stay on the tile kernels)
    s.res_fold = s.res == RES_ROWS && !c.no_res_fold && i > 0 && rn.fold_ok && w_direct(rn.block1);
    // a stage's first norm1 comes out of the resnet's last launch: as fp16 planes from the row-owning kernels' epilogue, as fp32
    // rows from the split-K reduce tail (what the split-K blocks read)
    s.ln_fold = !c.no_ln_fold && (s.res == RES_ONE ? s.rows : s.res == RES_ROWS ? s.rows && rn.block2.w2 && w_direct(rn.block2)
                                                                                 : r.sk_blocks && planes(rn.block2));
    // ... and its q | k | v too, in the full-chip regime of the row-owning blocks (no column split)
    s.qkv_fold = s.res == RES_ONE && s.ln_fold && !c.no_res_qkv && r.qkv_split <= 1 && e.blk[i][0].qkv_wf;
  }
  return r;
}

namespace {

ConvGemmArgs base_args(const Geo& g, const float* A, int lda, const GemmW& w, float* out, int ldo) {
  ConvGemmArgs a;
  conv_gemm_defaults(a);
  a.A = A; a.lda = lda; a.a_rows = g.a_rows; a.M = (int)g.M;
  a.Cin = w.Cin; a.ntaps = w.ntaps; a.tap_row0 = 0; a.tap_dil = 1;
  a.W = w.w; a.ldw = w.ldw; a.n_rows_w = w.n_rows; a.N = w.N; a.bias = w.bias;
  a.W3 = w.w3; a.w3_plane = (long)w.n_rows * w.ldw;
  a.out = out; a.ldo = ldo;
  a.alg_rows = g.frames();
  return a;
}

// (profiler: the estimator's Conv1d stack -- resnets, down / up / final convolutions, final projection -- is summed as one
// group; BASELINE.json's north star quotes an HBM fraction for it)
struct ConvStackScope {
  bool on;
  ConvStackScope() : on(prof_on()) { if (on) prof_group("flow_conv_stack"); }
  ~ConvStackScope() { if (on) prof_group(nullptr); }
};

// one estimator evaluation: what every launch of the call shares
struct Est {
  Context& c; FlowWs& w; const EstimatorW& e;
  const Geo& g; const EstRoute& rt; hipStream_t st;
  const EstTap* tap;      // jv_flow_estimator_tap (else null): run() returns behind this stage's launches
  bool tapped = false;    // ... and has copied its buffer out
  const long R = w.rows_alloc;          // rows of every workspace buffer (plane stride of the fp16 images kept in them)
  // every launcher of a call takes the route's product count in its argument record (`np`: read only where the launch runs fp16x3)
  int conv(ConvGemmArgs& a) { a.np = rt.np; return conv_gemm(a, 1, st); }
  float* const skip = w.cat + 256;      // columns [256,512) of the concat buffer

  // ---- trunk convolutions: fp16x3 from the measured bound of the trunk buffers (not for A = xin, which assemble_xin writes)
  // (zeroed by the caller once per solve, not per call: in the first launch after a reset every wave sends its atomic --
  // the per-CU L1 keeps serving the value the slot had at kernel start -- which cost 2.4 ms per step when done ten times)
  float* slots_of(const float* buf) const {
    if (buf == w.h) return w.amax;
    if (buf == w.h2) return w.amax + w.amax_stride;
    if (buf == w.cat || buf == skip) return w.amax + 2 * w.amax_stride;
    return nullptr;
  }
  void amax_geo(ConvGemmArgs& a) const {
    a.amax_G = FLOW_G; a.amax_S = g.S; a.amax_nb = g.B2; a.amax_mask = w.rowmask;
    a.amax_rows = g.uoff ? w.row_sample : nullptr;      // compact geometry: a row's slot by table
  }
  // every launch that writes a trunk buffer tracks max |value| into that buffer's slots (nothing consumes them in exact-range mode)
  void track(ConvGemmArgs& a) const {
    if (rt.exact) return;
    a.amax_out = slots_of(a.out);
    amax_geo(a);
  }
  void h3m(ConvGemmArgs& a, const GemmW& m) const {
    if (rt.exact || !m.w2 || a.A == w.xin || !slots_of(a.A)) return;
    a.W2 = m.w2; a.w2_plane = (long)m.n_rows * m.ldw; a.colscale = m.colscale; a.amax_in = slots_of(a.A); a.a_extra = 0.f;
    amax_geo(a);
  }
  void ln_mish(ConvGemmArgs& a, const LnW& n) const {      // ... -> LayerNorm -> Mish -> mask, in the launch's epilogue
    a.ln = 1; a.ln_g = n.g; a.ln_b = n.b; a.ln_eps = 1e-5f; a.act = ACT_MISH; a.rowmask_out = w.rowmask;
  }
  void causal3(ConvGemmArgs& a) const { a.tap_row0 = -2; a.rowmask_in = w.rowmask; }   // CausalConv1d k=3: rows t-2, t-1, t of the masked input
  // `a`: the full-semantics launch (N = 256); ln2 / out2: optional LayerNorm of the stored row for the next GEMM
  int splitk(const ConvGemmArgs& a, const LnW* ln2, float* out2) {
    ConvGemmArgs f = a;
    f.np = rt.np;
    return conv_splitk(f, rt.ksplit, w.partial, w.row_sample, ln2 ? ln2->g : nullptr, ln2 ? ln2->b : nullptr, out2, st);
  }
  // A causal k = 3 convolution to 256 channels, by the route: split-K tiles at short M, the row-owning kernel where the batch
  // fills the chip and the input has a tracked bound, else the tile kernels.
  // `follow` (Stage::ln_fold): the transformer block whose norm1 reads this convolution's output (a resnet's second
  // convolution): the launch writes it into w.ln too -- RowConvArgs::ln2_out, or the split-K reduce tail.
  // `fold` (Stage::res_fold): the resnet whose block1 this is -- its 1 x 1 res_conv (which reads the same rows) rides along as
  // a fourth fragment step per chunk and lands in w.res (RowConvArgs::res_out)
  int conv3(ConvGemmArgs& a, const GemmW& m, const BtbW* follow = nullptr, const ResnetW* fold = nullptr) {
    if (rt.ksplit > 1 && (a.W3 || a.W2) && (a.ldw & 7) == 0) return splitk(a, follow ? &follow->n1 : nullptr, w.ln);
    if (!rt.rows || !a.amax_in) return conv(a);
    RowConvArgs r{};
    r.np = rt.np;
    r.A = a.A; r.lda = a.lda; r.a_rows = a.a_rows; r.M = a.M; r.Cin = a.Cin; r.rowmask_in = a.rowmask_in;
    r.W2 = m.w2; r.w2_plane = (long)m.n_rows * m.ldw; r.ldw = m.ldw; r.colscale = m.colscale;
    r.Wf = m.wf; r.wf_plane = (long)m.N * m.ntaps * m.Cin;
    r.amax_in = a.amax_in; r.row_slot = w.row_sample; r.bias = a.bias;
    r.slot_G = FLOW_G; r.slot_S = g.uoff ? -1 : g.S; r.slot_nb = g.B2;      // = row_sample, by arithmetic (row_meta lays utterance b at G + b S; compact: by table)
    r.out = a.out; r.ldo = a.ldo;
    r.ln = a.ln; r.ln_g = a.ln_g; r.ln_b = a.ln_b; r.ln_eps = a.ln_eps; r.act = a.act; r.rowmask_out = a.rowmask_out;
    r.rowvec = a.rowvec; r.rowvec_ld = a.rowvec_ld; r.res = a.res1; r.ldr = a.ldr1;
    r.amax_out = a.amax_out; r.row_mask = w.rowmask;
    r.alg_rows = a.alg_rows;
    if (fold) {
      r.Wf = fold->wf4; r.wf_plane = 256L * 4 * a.Cin;
      r.res_out = w.res; r.res_cs = fold->res.colscale; r.res_bias = fold->res.bias;
    }
    if (follow) {
      r.ln2_out = reinterpret_cast<unsigned short*>(w.ln); r.ln2_plane = R * 256;
      r.ln2_g = follow->n1.g; r.ln2_b = follow->n1.b; r.ln2_scale = follow->qkv.a_scale;
    }
    if (tuning_env("JV_RB_STAMPS")) JV_TRY(arm_stamps(&w.rc_stamps, 1, 8, &r.stamps, 0));
    return rowconv(r, st);
  }
  // tuning builds (JV_RB_STAMPS): the phase stamps of the last rowconv / rowblock launch; est_stamps_dump prints their medians
  int arm_stamps(unsigned long long** buf, int sets, int n, unsigned long long** out, int set) {
    if (!*buf) JV_TRY(ws_alloc(c, (size_t)sets * 1024 * n * sizeof(unsigned long long), reinterpret_cast<void**>(buf)));
    *out = *buf + (size_t)set * 1024 * n;
    JV_HIP(hipMemsetAsync(*out, 0, (size_t)1024 * n * sizeof(unsigned long long), st));      // the stamps are atomic maxima
    return JV_OK;
  }

  // CausalResnetBlock1D (decoder.py:110-115, 784-795) of stage i, in -> out [*,256]; out == in except on the whole-resnet launch
  int resnet(int i, const float* in, int ldin, float* out) {
    ConvStackScope scope;
    const ResnetW& r = e.res[i];
    const EstRoute::Stage& s = rt.stage[i];
    const BtbW* follow = s.ln_fold ? &e.blk[i][0] : nullptr;
    if (s.res == RES_ONE) {
      if (out == in) return fail(JV_ERR_STATE, "flow: the whole-resnet launch cannot run in place");
      RowResArgs a{};
      a.np = rt.np;
      a.A = in; a.lda = ldin; a.a_rows = g.a_rows; a.M = (int)g.M; a.Cin = ldin; a.rowmask = w.rowmask;
      a.amax_in = slots_of(in); a.slot_G = FLOW_G; a.slot_S = g.uoff ? -1 : g.S; a.slot_nb = g.B2; a.row_slot = w.row_sample;
      a.Wf1 = r.wf4; a.wf1_plane = 256L * 4 * ldin;
      a.cs1 = r.block1.colscale; a.b1 = r.block1.bias; a.ln1_g = r.ln1.g; a.ln1_b = r.ln1.b;
      a.csr = r.res.colscale; a.br = r.res.bias;
      a.temb = w.temb + i * 256; a.h2_bound = r.h2_bound; a.ln_eps = 1e-5f;
      a.Wf2 = r.block2.wf; a.wf2_plane = 256L * 3 * 256;
      a.cs2 = r.block2.colscale; a.b2 = r.block2.bias; a.ln2_g = r.ln2.g; a.ln2_b = r.ln2.b;
      a.out = out; a.ldo = 256; a.amax_out = slots_of(out);
      a.alg_rows = g.frames();
      if (follow) {
        a.lnf_g = follow->n1.g; a.lnf_b = follow->n1.b; a.lnf_scale = follow->qkv.a_scale;
        if (!s.qkv_fold) {
          a.lnf_out = reinterpret_cast<unsigned short*>(w.ln); a.lnf_plane = R * 256;
        } else {      // ... and its to_q | to_k | to_v over those planes, which then never leave LDS (block_rows' buffers and scales)
          a.Wqf = follow->qkv.wf; a.wqf_plane = (long)follow->qkv.N * follow->qkv.Cin; a.csq = follow->qkv.colscale;
          a.q = w.qkv; a.kv2 = reinterpret_cast<unsigned short*>(w.qkv + R * 512); a.kv2_plane = R * 1024;
          a.k_scale = follow->k_scale; a.v_scale = follow->v_scale;
        }
      }
      return rowres(a, st);
    }
    // block1 writes w.h2 (never the input's buffer: est_route); block2 writes `out` only after block1 and res_conv have consumed `in`
    if (in == w.h2) return fail(JV_ERR_STATE, "flow: a resnet's input sits in the buffer its first convolution writes");
    ConvGemmArgs a = base_args(g, in, ldin, r.block1, w.h2, 256);
    causal3(a);
    ln_mish(a, r.ln1);
    a.rowvec = w.temb + i * 256; a.row_sample = w.row_sample; a.rowvec_ld = g.temb_pre ? 0 : EST_NRES * 256;      // (0: one embedding for all rows)
    h3m(a, r.block1);
    track(a);      // -> h2
    JV_TRY(conv3(a, r.block1, nullptr, s.res_fold ? &r : nullptr));
    if (!s.res_fold) {      // (the tile kernels' route, the first resnet -- its input has no measured bound --, JV_NO_RES_FOLD=1)
      a = base_args(g, in, ldin, r.res, w.res, 256);
      a.rowmask_in = w.rowmask;
      h3m(a, r.res);
      JV_TRY(conv(a));
    }
    a = base_args(g, w.h2, 256, r.block2, out, 256);
    causal3(a);
    ln_mish(a, r.ln2);
    a.res1 = w.res; a.ldr1 = 256;
    h3m(a, r.block2);
    track(a);      // -> h
    return conv3(a, r.block2, follow);
  }

  // ---- BasicTransformerBlock (transformer.py:355-443) on the tile kernels: h -> h, last GEMM may retarget its output
  // the four linears of a block run fp16x3 when registry.hip proved their input range (GemmW::a_scale)
  void h3(ConvGemmArgs& a, const GemmW& m) const {
    if (rt.exact || !m.w2 || !(m.a_scale > 0.f)) return;
    a.W2 = m.w2; a.w2_plane = (long)m.n_rows * m.ldw; a.colscale = m.colscale; a.a_scale = m.a_scale;
  }
  // ... and then take their A operand as the fp16 planes their producer wrote into the same buffer (same bytes as fp32)
  bool pre(const GemmW& m) const { return rt.pre_planes && m.w2 && m.a_scale > 0.f; }
  void planes_in(ConvGemmArgs& a, float* buf, int C) const { a.A2 = reinterpret_cast<const unsigned short*>(buf); a.a2_plane = R * C; a.lda2 = C; }
  int ln_to(const LnW& n, const GemmW& m, const float* h) {
    if (pre(m)) return layernorm256_planes(h, reinterpret_cast<unsigned short*>(w.ln), R * 256, m.a_scale, n.g, n.b, 1e-5f, g.M, st);
    return layernorm_rows(h, nullptr, w.ln, n.g, n.b, 1e-5f, g.M, 256, nullptr, st);
  }
  int block_tiles(const BtbW& b, const BtbW* next, bool ln_ready, float* h, float* out, int ldo) {
    const bool sk = rt.sk_blocks;      // split-K tails also write the next LayerNorm (fp32 rows) into w.ln
    if (!(sk && ln_ready)) JV_TRY(ln_to(b.n1, b.qkv, h));
    ConvGemmArgs a = base_args(g, w.ln, 256, b.qkv, w.qkv, 1536);
    h3(a, b.qkv);
    if (pre(b.qkv)) planes_in(a, w.ln, 256);
    JV_TRY(conv(a));
    AttnArgs at{};
    at.np = rt.np;
    at.qkv = w.qkv; at.ld = 1536; at.k_off = 512; at.v_off = 1024; at.out = w.att; at.ldo = 512;
    at.B = g.B2; at.H = EST_HEADS; at.G = FLOW_G; at.S = g.S; at.L = g.T; at.lens = w.lens2;
    at.chunk = rt.attn_chunk;
    if (!rt.exact && b.q_scale > 0.f) { at.q_scale = b.q_scale; at.k_scale = b.k_scale; at.v_scale = b.v_scale; }
    if (pre(b.out)) { at.out2 = reinterpret_cast<unsigned short*>(w.att); at.out2_plane = R * 512; at.out2_scale = b.out.a_scale; }
    JV_TRY(attention64(at, st));
    a = base_args(g, w.att, 512, b.out, h, 256);
    a.res1 = h; a.ldr1 = 256;
    track(a);      // -> h
    h3(a, b.out);
    if (pre(b.out)) planes_in(a, w.att, 512);
    if (sk) {
      JV_TRY(splitk(a, &b.n3, w.ln));      // h += to_out(att); ln = LayerNorm3(h)
    } else {
      JV_TRY(conv(a));
      JV_TRY(ln_to(b.n3, b.ff1, h));
    }
    a = base_args(g, w.ln, 256, b.ff1, w.ff, 1024);
    a.act = ACT_GELU;
    h3(a, b.ff1);
    if (pre(b.ff1)) planes_in(a, w.ln, 256);
    if (pre(b.ff2) && a.W2) {      // the GELU epilogue writes ff2's operand (plane output exists on the fp16x3 lean path)
      a.out2 = reinterpret_cast<unsigned short*>(w.ff); a.out2_plane = R * 1024; a.ldo2 = 1024; a.out2_scale = b.ff2.a_scale;
    }
    const bool ff_planes = a.out2 != nullptr;
    JV_TRY(conv(a));
    a = base_args(g, w.ff, 1024, b.ff2, out, ldo);
    a.res1 = h; a.ldr1 = 256;
    track(a);      // -> h / cat
    h3(a, b.ff2);
    if (ff_planes) planes_in(a, w.ff, 1024);
    if (sk) return splitk(a, (next && out == h) ? &next->n1 : nullptr, w.ln);      // + the next block's norm1
    return conv(a);
  }

  // ---- the same block on the row-owning GEMM (rowgemm_kernel.h) when the batch fills the chip: every linear takes its A
  // operand as the fp16 planes its producer wrote (LayerNorm, attention, the previous linear's epilogue), to_out and
  // ff.net.2 add the residual AND run the LayerNorm that follows in their epilogue, ff.net.0 applies GELU and writes
  // ff.net.2's operand: four GEMM launches + attention per block -- or to_out, the feed-forward and the next q | k | v in one
  // (rowblock_kernel.h) -- and no stand-alone row-wise kernel except the first LayerNorm of a stage.
  RowGemmArgs rg_args(const float* planes, int K, const GemmW& m) const {
    RowGemmArgs a{};
    a.A2 = reinterpret_cast<const unsigned short*>(planes); a.a2_plane = R * K; a.a_rows = g.a_rows; a.lda2 = K;
    a.M = (int)g.M; a.K = K; a.N = m.N;
    a.W2 = m.w2; a.w2_plane = (long)m.n_rows * m.ldw; a.ldw = m.ldw; a.colscale = m.colscale; a.a_scale = m.a_scale;
    a.Wf = m.wf; a.wf_plane = (long)m.N * m.Cin;
    a.bias = m.bias; a.ln_eps = 1e-5f; a.out2_scale = 1.f;
    a.alg_rows = g.frames();
    a.np = rt.np;
    return a;
  }
  void rg_track(RowGemmArgs& a) const { a.amax_out = slots_of(a.out); a.row_slot = w.row_sample; a.row_mask = w.rowmask; }
  // to_out -> LayerNorm3 -> feed-forward (-> the next block's LayerNorm1 -> q | k | v) in ONE launch?
  bool fused(const BtbW& b) const { return rt.block_fuse && b.block_wf; }
  // ... which then leaves the next block's q | k | v behind, unless its column chunks are dealt out (qkv_split)
  bool qkv_rides(const BtbW& b) const { return fused(b) && rt.qkv_split <= 1; }
  // `next`: the block that follows in the same stage (its norm1 runs in this block's last epilogue)
  // `ln_ready` / `qkv_ready`: this block's norm1 planes / q | k | v were produced by the launch before it
  int block_rows(const BtbW& b, const BtbW* next, bool ln_ready, bool qkv_ready, float* h, float* out, int ldo) {
    if (!ln_ready && !qkv_ready)
      JV_TRY(layernorm256_planes(h, reinterpret_cast<unsigned short*>(w.ln), R * 256, b.qkv.a_scale, b.n1.g, b.n1.b, 1e-5f, g.M, st));
    // q | k | v = to_q/k/v(ln): q as fp32 rows [R,512] at the head of the qkv buffer, k and v as fp16 planes [2][R][1024]
    // behind it (same bytes as [R,1536] fp32), scaled for the attention kernel, which then splits nothing
    unsigned short* const kv2 = reinterpret_cast<unsigned short*>(w.qkv + R * 512);
    RowGemmArgs a;
    if (!qkv_ready) {
      a = rg_args(w.ln, 256, b.qkv);
      a.nsplit = rt.qkv_split; a.rt = rt.qkv_rt;
      a.out = w.qkv; a.ldo = 512;
      a.out2 = kv2; a.out2_plane = R * 1024; a.ldo2 = 1024; a.out2_scale = b.k_scale; a.out2_scale2 = b.v_scale;
      JV_TRY(rowgemm(a, RG_QKV, st));
    }
    AttnArgs at{};
    at.np = rt.np;
    at.qkv = w.qkv; at.out = w.att; at.ldo = 512;
    at.B = g.B2; at.H = EST_HEADS; at.G = FLOW_G; at.S = g.S; at.L = g.T; at.lens = w.lens2; at.uoff = g.uoff;
    at.chunk = rt.attn_chunk;
    at.q_scale = b.q_scale; at.k_scale = b.k_scale; at.v_scale = b.v_scale;
    at.out2 = reinterpret_cast<unsigned short*>(w.att); at.out2_plane = R * 512; at.out2_scale = b.out.a_scale;
    at.ld = 512; at.kv2 = kv2; at.kv2_plane = R * 1024; at.kv_ld = 1024;
    // whole-utterance attention of a batch that fills its rounds: one wave per SIMD, 160 queries per wave; else attn64_pl
    if (rt.attn_single && attention64_single_fits(at)) JV_TRY(attention64_single(at, st));
    else JV_TRY(attention64_planes(at, st));
    const bool follows = next && out == h;
    if (fused(b)) {      // the LayerNorm planes never leave LDS (rowblock_kernel.h)
      RowBlockArgs f{};
      f.np = rt.np;
      f.A2 = reinterpret_cast<const unsigned short*>(w.att); f.a2_plane = R * 512; f.a_rows = g.a_rows; f.M = (int)g.M;
      f.Wof = b.out.wf; f.wof_plane = (long)b.out.N * b.out.Cin; f.cso = b.out.colscale; f.bo = b.out.bias; f.a_scale_o = b.out.a_scale;
      f.h = h; f.ln3_g = b.n3.g; f.ln3_b = b.n3.b;
      f.W1f = b.ff1.wf; f.w1f_plane = (long)b.ff1.N * b.ff1.Cin; f.cs1 = b.ff1.colscale; f.b1 = b.ff1.bias; f.a_scale1 = b.ff1.a_scale;
      f.h_scale = b.ff2.a_scale;
      f.W2f = b.ff2.wf; f.w2f_plane = (long)b.ff2.N * b.ff2.Cin; f.cs2 = b.ff2.colscale; f.b2 = b.ff2.bias;
      f.out = out; f.ldo = ldo;
      f.amax_h = slots_of(h); f.amax_out = slots_of(out); f.row_slot = w.row_sample; f.row_mask = w.rowmask;
      f.alg_rows = g.frames();
      const bool qkv = follows && qkv_rides(b);
      if (follows) { f.ln1_g = next->n1.g; f.ln1_b = next->n1.b; f.a_scale_q = next->qkv.a_scale; }
      if (qkv) {
        f.Wqf = next->qkv.wf; f.wqf_plane = (long)next->qkv.N * next->qkv.Cin; f.csq = next->qkv.colscale;
        f.q = w.qkv; f.kv2 = kv2; f.kv2_plane = R * 1024; f.k_scale = next->k_scale; f.v_scale = next->v_scale;
      } else if (follows) {
        // few row tiles: the next block's LayerNorm1 planes leave through HBM and its q | k | v runs as its own launch with
        // the column chunks dealt over the idle CUs (qkv_split, est_route)
        f.ln_out = reinterpret_cast<unsigned short*>(w.ln); f.ln_out_plane = R * 256;
      }
      if (tuning_env("JV_RB_STAMPS")) JV_TRY(arm_stamps(&w.rb_stamps, 2, 48, &f.stamps, qkv ? 0 : 1));
      return rowblock(f, qkv, st);
    }
    a = rg_args(w.att, 512, b.out);      // h += to_out(att); ln = LayerNorm3(h)
    a.out = h; a.ldo = 256; a.res = h; a.ldr = 256;
    a.out2 = reinterpret_cast<unsigned short*>(w.ln); a.out2_plane = R * 256; a.ldo2 = 256; a.out2_scale = b.ff1.a_scale;
    a.ln_g = b.n3.g; a.ln_b = b.n3.b;
    rg_track(a);
    JV_TRY(rowgemm(a, RG_RES_LN, st));
    if (rt.ffn_fuse && b.ffn_wf) {
      // the feed-forward pair in one launch (rowffn_kernel): the 1024-wide hidden tile never leaves LDS
      RowFfnArgs f{};
      f.np = rt.np;
      f.A2 = reinterpret_cast<const unsigned short*>(w.ln); f.a2_plane = R * 256; f.a_rows = g.a_rows; f.lda2 = 256; f.M = (int)g.M;
      f.W1f = b.ff1.wf; f.w1f_plane = (long)b.ff1.N * b.ff1.Cin; f.cs1 = b.ff1.colscale; f.b1 = b.ff1.bias; f.a_scale1 = b.ff1.a_scale;
      f.h_scale = b.ff2.a_scale;
      f.W2f = b.ff2.wf; f.w2f_plane = (long)b.ff2.N * b.ff2.Cin; f.cs2 = b.ff2.colscale; f.b2 = b.ff2.bias;
      f.out = out; f.ldo = ldo; f.res = h; f.ldr = 256;
      f.ln_eps = 1e-5f; f.out2_scale = 1.f;
      f.amax_out = slots_of(out); f.row_slot = w.row_sample; f.row_mask = w.rowmask;
      f.alg_rows = g.frames();
      if (follows) {
        f.ln = 1; f.out2 = reinterpret_cast<unsigned short*>(w.ln); f.out2_plane = R * 256; f.ldo2 = 256; f.out2_scale = next->qkv.a_scale;
        f.ln_g = next->n1.g; f.ln_b = next->n1.b;
      }
      return rowffn(f, st);
    }
    a = rg_args(w.ln, 256, b.ff1);       // ff = gelu(ff.net.0(ln))
    a.out2 = reinterpret_cast<unsigned short*>(w.ff); a.out2_plane = R * 1024; a.ldo2 = 1024; a.out2_scale = b.ff2.a_scale;
    JV_TRY(rowgemm(a, RG_GELU_PL, st));
    a = rg_args(w.ff, 1024, b.ff2);      // out = h + ff.net.2(ff); the next block's norm1 of it
    a.out = out; a.ldo = ldo; a.res = h; a.ldr = 256;
    rg_track(a);
    if (follows) {
      a.out2 = reinterpret_cast<unsigned short*>(w.ln); a.out2_plane = R * 256; a.ldo2 = 256; a.out2_scale = next->qkv.a_scale;
      a.ln_g = next->n1.g; a.ln_b = next->n1.b;
      return rowgemm(a, RG_RES_LN, st);
    }
    return rowgemm(a, RG_RES, st);
  }

  // jv_flow_estimator_tap: stage `id` stands in columns [0, C) of `buf` -- if it is the tap, out it goes, channels first, zeros at and
  // behind every sample's clamped length (either geometry)
  int stage_done(int id, const float* buf, int ld, int C = 256) {
    if (!tap || tap->id != id) return JV_OK;
    tapped = true;
    return rows_to_cf(buf, ld, 0, FLOW_G, g.S, tap->out, (long)C * g.T, g.B2, C, g.T, w.lens2, st, g.uoff);
  }
  static int tap_res(int i) { return i == 0 ? JV_EST_TAP_RES0 : JV_EST_TAP_RES1 + JV_EST_TAP_PER_STAGE * (i - 1); }

  // the four blocks of stage i on the trunk buffer h; the last one may retarget its output (skip / concat buffer)
  int blocks(int i, float* h, float* last_out, int last_ldo) {
    const EstRoute::Stage& s = rt.stage[i];
    const BtbW* blk = e.blk[i];
    if (rt.compact && !s.rows) return fail(JV_ERR_STATE, "flow: the compact geometry exists on the row-owning kernels only");
    bool qkv_ready = s.qkv_fold;
    for (int j = 0; j < EST_NBLK; ++j) {
      const bool last = j == EST_NBLK - 1;
      const BtbW* next = last ? nullptr : &blk[j + 1];
      float* const out = last ? last_out : h;
      const int ldo = last ? last_ldo : 256;
      if (s.rows) {
        JV_TRY(block_rows(blk[j], next, j > 0 || s.ln_fold, qkv_ready, h, out, ldo));
        qkv_ready = !last && qkv_rides(blk[j]);
      } else {
        JV_TRY(block_tiles(blk[j], next, j > 0 || s.ln_fold, h, out, ldo));
      }
      JV_TRY(stage_done(tap_res(i) + 1 + j, out, ldo));
      if (tapped) return JV_OK;
    }
    return JV_OK;
  }

  // a trunk convolution between the stages (down / up / final), optionally with the final block's LayerNorm + Mish + mask
  int trunk_conv(const GemmW& m, const float* in, int ldin, float* out, const LnW* ln = nullptr) {
    ConvGemmArgs a = base_args(g, in, ldin, m, out, 256);
    causal3(a);
    if (ln) ln_mish(a, *ln);
    h3m(a, m);
    track(a);
    return conv3(a, m);
  }

  // the network (decoder.py:917-1018)
  int run() {
    // timestep embedding: sinusoid -> Linear+SiLU -> Linear (+Mish, the only consumer) -> 14 projections
    if (!g.temb_pre) JV_TRY(time_embedding(c, g.t_ptr, g.t_stride, g.B2, w.tsin, w.t1, w.tmish, w.temb, st, est_tap_time_stages(tap)));
    if (tap && tap->id <= JV_EST_TAP_TEMB) {      // [n, C] rows as they stand: one per sample, or the step's one (temb_pre)
      float* const bufs[4] = {w.tsin, w.t1, w.tmish, w.temb};
      JV_HIP(hipMemcpyAsync(tap->out, bufs[tap->id], sizeof(float) * (g.temb_pre ? 1 : g.B2) * est_tap_channels(tap->id),
                            hipMemcpyDeviceToDevice, st));
      return JV_OK;
    }
    // down: resnet -> 4 blocks (result doubles as the skip) -> causal conv
    JV_TRY(resnet(0, w.xin, 320, w.h));
    JV_TRY(stage_done(tap_res(0), w.h, 256));
    if (tapped) return JV_OK;
    JV_TRY(blocks(0, w.h, skip, 512));
    if (tapped) return JV_OK;
    { ConvStackScope scope; JV_TRY(trunk_conv(e.down_conv, skip, 512, w.h)); }
    JV_TRY(stage_done(JV_EST_TAP_DOWN, w.h, 256));
    if (tapped) return JV_OK;
    // mid x12; the last block writes straight into columns [0,256) of the concat buffer.  On the whole-resnet launch the trunk
    // alternates between w.h and w.h2 (est_route: all twelve or none), and is back in w.h after the twelfth
    float* trunk = w.h;
    for (int i = 1; i <= EST_NMID; ++i) {
      float* const dst = rt.stage[i].res != RES_ONE ? trunk : trunk == w.h ? w.h2 : w.h;
      JV_TRY(resnet(i, trunk, 256, dst));
      trunk = dst;
      JV_TRY(stage_done(tap_res(i), trunk, 256));
      if (tapped) return JV_OK;
      JV_TRY(blocks(i, trunk, i == EST_NMID ? w.cat : trunk, i == EST_NMID ? 512 : 256));
      if (tapped) return JV_OK;
    }
    if (trunk != w.h) return fail(JV_ERR_STATE, "flow: the mid stages left the trunk in the scratch buffer");
    // up: resnet(cat[x, skip]) -> 4 blocks -> causal conv -> final block -> 1x1 projection
    JV_TRY(resnet(EST_NRES - 1, w.cat, 512, w.h));
    JV_TRY(stage_done(tap_res(EST_NRES - 1), w.h, 256));
    if (tapped) return JV_OK;
    JV_TRY(blocks(EST_NRES - 1, w.h, w.h, 256));
    if (tapped) return JV_OK;
    ConvStackScope scope;
    JV_TRY(trunk_conv(e.up_conv, w.h, 256, w.h2));
    JV_TRY(stage_done(JV_EST_TAP_UPC, w.h2, 256));
    if (tapped) return JV_OK;
    JV_TRY(trunk_conv(e.final_conv, w.h2, 256, w.h, &e.final_ln));
    JV_TRY(stage_done(JV_EST_TAP_FIN, w.h, 256));
    if (tapped) return JV_OK;
    ConvGemmArgs a = base_args(g, w.h, 256, e.final_proj, w.d, 80);
    a.rowmask_in = w.rowmask;
    a.rowmask_out = w.rowmask;
    h3m(a, e.final_proj);
    JV_TRY(conv(a));
    return stage_done(JV_EST_TAP_D, w.d, 80, 80);
  }
};

}  // namespace

// timestep embedding of n timesteps t[i * t_stride]: sinusoid -> Linear + SiLU -> Linear (+ Mish, the only consumer) -> the 14
// resnets' projections, emb [n, 14 * 256] (decoder.py:917-935, 98-108).  Rows are independent: a row's bits do not depend on n.
// stages < 4 (jv_flow_estimator_tap): the first so many of the four launches
int time_embedding(Context& c, const float* t, int t_stride, int n, float* sin_buf, float* h1, float* hm, float* emb, hipStream_t st,
                   int stages) {
  const EstimatorW& e = c.est;
  JV_TRY(time_sinusoid(t, t_stride, c.flow->tfreq, sin_buf, n, st));
  if (stages < 2) return JV_OK;
  Geo tg{n, 1, 1, n, n, nullptr, 1};
  ConvGemmArgs a = base_args(tg, sin_buf, 320, e.time1, h1, 1024);
  a.act = ACT_SILU;
  JV_TRY(conv_gemm(a, 1, st));
  if (stages < 3) return JV_OK;
  a = base_args(tg, h1, 1024, e.time2, hm, 1024);
  a.act = ACT_MISH;
  JV_TRY(conv_gemm(a, 1, st));
  if (stages < 4) return JV_OK;
  a = base_args(tg, hm, 1024, e.temb_all, emb, EST_NRES * 256);
  return conv_gemm(a, 1, st);
}

// channels of a tap's buffer (0: no such tap)
int est_tap_channels(int id) {
  if (id < 0 || id >= JV_EST_TAP_COUNT) return 0;
  switch (id) {
    case JV_EST_TAP_TSIN: case JV_EST_TAP_XIN: return 320;
    case JV_EST_TAP_T1: case JV_EST_TAP_TMISH: return 1024;
    case JV_EST_TAP_TEMB: return EST_NRES * 256;
    case JV_EST_TAP_D: return 80;
  }
  return 256;
}

int est_tap_time_stages(const EstTap* tap) { return tap && tap->id <= JV_EST_TAP_TEMB ? tap->id + 1 : 4; }

int est_tap_check(const EstTap* tap, int ns, int nt, int T) {
  if (!tap) return JV_OK;
  const int C = est_tap_channels(tap->id);
  if (!C) return fail(JV_ERR_ARG, "jv_flow_estimator_tap: unknown tap");
  if (!tap->out) return fail(JV_ERR_ARG, "jv_flow_estimator_tap: null out");
  const long need = tap->id <= JV_EST_TAP_TEMB ? (long)nt * C : (long)ns * C * T;
  if (tap->out_floats < need)
    return fail(JV_ERR_SHAPE, "jv_flow_estimator_tap: out holds fewer floats than the tap ([n, C] for the time taps, else [samples, C, T])");
  return JV_OK;
}

int estimator_body(Context& c, const Geo& g, const EstRoute& rt, hipStream_t st, const EstTap* tap) {
  return Est{c, *c.flow, c.est, g, rt, st, tap}.run();
}

#ifdef JV_TUNING
// tuning aid (JV_RB_STAMPS): phase breakdown of the LAST rowblock launch (with and without q|k|v) and rowconv launch of a solve
int est_stamps_dump(Context& c, const Geo& g, hipStream_t st) {
  FlowWs& w = *c.flow;
  if (!w.rb_stamps || !tuning_env("JV_RB_STAMPS")) return JV_OK;
  JV_HIP(hipStreamSynchronize(st));
  const int nwg = (int)std::min<long>(1024, cdivl(g.M, 16 * std::max(1, rowgemm_tile((int)g.M))));
  auto dump = [&](const char* what, const unsigned long long* dev, int n) -> int {
    std::vector<unsigned long long> hs((size_t)nwg * n);
    JV_HIP(hipMemcpy(hs.data(), dev, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    fprintf(stderr, "[%s] %d workgroups; median s_memtime ticks (100 MHz) since start:", what, nwg);
    for (int i = 1; i < n; ++i) {
      std::vector<long> d;
      for (int b = 0; b < nwg; ++b)
        if (hs[(size_t)b * n + i] > hs[(size_t)b * n]) d.push_back((long)(hs[(size_t)b * n + i] - hs[(size_t)b * n]));
      std::sort(d.begin(), d.end());
      if (!d.empty()) fprintf(stderr, " %d:%ld", i, d[d.size() / 2]);
    }
    fprintf(stderr, "\n");
    return JV_OK;
  };
  JV_TRY(dump("rowblock stamps,qkv", w.rb_stamps, 48));
  JV_TRY(dump("rowblock stamps", w.rb_stamps + 1024 * 48, 48));
  return w.rc_stamps ? dump("rowconv stamps", w.rc_stamps, 8) : JV_OK;
}
#endif

}  // namespace jv
