// Row-owning fp16x3 convolution for the vocoder's ResBlocks (jyutvoice/hifigan/generator.py:90-97: xt = Snake(x) ->
// Conv1d(C, C, k, dilation d) -> Snake -> Conv1d(C, C, k) -> x + xt, kernel sizes 3 / 7 / 11, dilations 1 / 3 / 5, at
// C = 256, 128, 64 channels and 8 T, 40 T, 120 T + 1 rows per utterance): the trunk's treatment (rowconv_kernel.h,
// rowgemm_wa_kernel) for the 72 convolutions that are 85 % of the vocoder's arithmetic.
//
// The tile kernels (conv_gemm_x6_kernel.h) restage a 32-channel slice of the window for every K chunk -- Snake (a sin^2 per
// element), the fp16 split, an LDS store, two barriers -- and stream the weights through LDS as well: 0.19 - 0.30 of the
// fp16x3 ceiling, the 64-channel stage lowest (1.15 M rows of it).  Here one 8-wave workgroup owns 80 NG rows x all C output
// channels (NG = 256 / C row groups of 80 rows: every wave a 80 x 32 tile, 30 MFMAs per 32-deep step, as in the trunk):
//   * the WHOLE window -- 80 NG + (k - 1) d rows x C channels -- goes through Snake and the plane split ONCE, into LDS
//     (130 x 256, 210 x 128 or 370 x 64 values: 93 - 139 KB), and every tap of every chunk reads it in place at a row offset:
//     no staging, no DMA and no barrier inside the main loop;
//   * the weights arrive in fragment order through the register double buffer with hand-counted waits (WFragBuf: row_mainloop.h);
//   * v_mfma_f32_16x16x32_f16; the epilogue (bias, residuals, scaling, accumulation, measured-bound tracking) runs per wave
//     through a private transposition patch, no workgroup barrier: one wave's stores run under the others' MFMAs.
// Arithmetic: the tile kernels' (same Snake evaluation, same per-utterance power-of-two scale from the measured bound, products
// hh' + hl' + lh' smallest first, fp32 accumulate over K ascending); 16x16x32 instead of 32x32x16 MFMAs sum a 32-deep step
// in another internal order, so results agree with the tile kernels to rounding.
#pragma once
#include "hift_common.h"

namespace jv {

struct HiftConvArgs {
  const float* A;                  // fp32 row buffer [rows, C]; output row m, tap j reads row m + tap_row0 + j dil
  long a_rows;                     // rows of A that may be read (others read as zero)
  int M;                           // output rows
  int ntaps, dil, tap_row0;
  const unsigned char* rowmask_in; // per A row or null: 0 -> the row reads as zero
  const float* alpha;              // Snake: x + sin^2(alpha x) / (alpha + 1e-9), per input channel
  const unsigned short* Wf;        // fp16 planes of W[n][j C + ci] * 2^e_n in fragment order (pack_wfrag over K = ntaps C)
  long wf_plane;
  const float* colscale;           // 2^-e_n
  const float* bias;
  const float* amax_in;            // per-utterance measured bound of A; scale = h3_scale_dev(amax_in[slot] + a_extra)
  float a_extra;                   // what Snake can add to |x|: max 1 / (alpha + 1e-9)
  int slot_G, slot_S, slot_nb;     // slot(row) = clamp((row - slot_G) / slot_S, 0, slot_nb - 1)
  const int* slot_map;             // or, when set: slot(row) = slot_map[row] (the compact geometry of ragged batches: a table per level)
  float* out;                      // [rows, C]:  out = ((acc + bias) + res1 + res2) * out_scale (+ previous out)
  const float *res1, *res2;        // [rows, C] or null (either may alias out)
  float out_scale;
  int accumulate;
  float* amax_out;                 // tracking of what is stored, per utterance slot; rows with amax_mask == 0 are padding
  const unsigned char* amax_mask;
  long alg_rows;
};

// NG row groups of 80 rows per workgroup; a workgroup has NG * C / 32 waves (each a 80 x 32 tile)
template <int NG> constexpr int hc_rows() { return HC_RG * NG; }
template <int C, int NG> constexpr int hc_threads() { return 64 * NG * (C / 32); }
template <int C, int NG> inline int hc_lds_bytes(int ntaps, int dil) { return hc_lds_layout<C, NG, false>(ntaps, dil).total; }

template <int C, int NG>
__global__ __launch_bounds__(64 * NG * (C / 32), 2) void hiftconv_kernel(const HiftConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hc_lds[];
  constexpr int RT = HC_RT, RG = HC_RG;
  constexpr int NCH = C / 32, CW = C / 32, R = RG * NG, NT = 64 * NG * CW;
  static_assert(R + 56 <= NT, "one window row per thread in the facts pass");
  typedef const __attribute__((address_space(1))) unsigned char* gbytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int grp = wave / CW, cp = wave % CW;    // row group, 32-column pair
  const int m0 = blockIdx.x * R;
  const int WR = R + (p.ntaps - 1) * p.dil;     // window rows really used
  const int WRP = ((WR + 7) & ~7) + 1;
  const int PS = WRP * 64, CS = 2 * PS;         // plane and chunk strides of the operand image
  const int KS = p.ntaps * NCH;                 // 32-deep steps (even: NCH is)
  const HcLds L = hc_lds_layout<C, NG, false>(p.ntaps, p.dil);
  float* const wscale = reinterpret_cast<float*>(hc_lds);                                   // [WRP]: < 0 = the row reads as zero
  int2* const rowinfo = reinterpret_cast<int2*>(hc_lds + L.rowinfo);                        // [R]
  unsigned char* const img = hc_lds + L.img;                                                // [NCH][2][WRP][64 B]
  float* const patch = reinterpret_cast<float*>(hc_lds + L.patch) + wave * (16 * 36);

  // ---- W: this wave's fragment stream through the register double buffer; steps 0 and 1 are requested here ----
  HcWeights<C> w;
  w.start(p.Wf, p.wf_plane, cp, lane);
  WFragBuf<2> bq;
  bq.zero();
  // the weights start first: everything below is global-load latency they spend in flight.  (A counted loop that the compiler
  // unrolls, on purpose: as straight-line steps, here or in the walker, the same loads leave hiftpair_kernel<128,2,11> with four
  // VGPRs more -- profiles/hift_common_isa.md)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    if (b == 0) { w.template load<0, 0>(bq); w.template load<0, 1>(bq); }
    if (b == 1) { w.template load<1, 0>(bq); w.template load<1, 1>(bq); }
    w.advance(KS);
  }

  // ---- per-row facts: the window rows' scales (one level of unconditional loads on clamped indices: rowconv_wd_kernel) ----
  auto slot_of = [&](const long row) { return hc_slot_of(p, row); };
  constexpr int RI_TRACK = HC_RI_TRACK;
  {
    // (WR <= R + 50 < NT: one window row and one output row per thread)
    const long ar = (long)m0 + p.tap_row0 + tid;
    const bool in_w = tid < WR && ar >= 0 && ar < p.a_rows;
    const long arc = ar < 0 ? 0 : (ar < p.a_rows ? ar : p.a_rows - 1);
    const int mk = ((gbytes)(p.rowmask_in ? p.rowmask_in : hc_ones_page))[p.rowmask_in ? arc : 0];
    const float am_w = p.amax_in[slot_of(arc)];
    const long mt = (long)m0 + (tid < R ? tid : 0);
    const long mc = mt < p.M ? mt : (long)p.M - 1;
    const int sl_o = slot_of(mc);
    const int trk = ((gbytes)(p.amax_mask ? p.amax_mask : hc_ones_page))[p.amax_mask ? mc : 0];
    const float am_o = p.amax_in[sl_o];
    if (tid < WRP) wscale[tid] = (in_w && mk != 0) ? h3_scale_dev(am_w + p.a_extra) : -1.f;
    if (tid < R) {
      const float inv = mt < p.M ? 1.0f / h3_scale_dev(am_o + p.a_extra) : 0.f;
      rowinfo[tid] = int2{(int)__float_as_uint(inv), sl_o | ((p.amax_out && mt < p.M && trk != 0) ? RI_TRACK : 0)};
    }
  }
  __syncthreads();

  // ---- the window, once: fp32 rows -> Snake -> x scale -> two fp16 planes, chunk-major operand image ----
  hc_stage_window<C, NT>(p.A + ((long)m0 + p.tap_row0) * C, WR, (const hc_lds_f32*)wscale, p.alpha, (hc_lds_u8*)img, CS, PS, tid);
  // the per-column constants of the epilogue, requested here so that their latency is not paid behind the main loop
  const int ncol = 32 * cp + 4 * (lane & 7);      // this lane's four columns in the row-wise passes
  rg_f32x4 cs4 = *reinterpret_cast<const rg_f32x4*>(p.colscale + ncol);
  rg_f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) b4 = *reinterpret_cast<const rg_f32x4*>(p.bias + ncol);
  wait_vmcnt<0>();
  bq.landed_all();
  lds_barrier();      // the operand image is complete: the only barrier ahead of the epilogue

  // ---- main loop: step ks = (tap j = ks / NCH, chunk c = ks % NCH); A fragments of row tile mt at window row
  // 80 grp + 16 mt + r16 + j dil (the 16-byte slot key depends on r16 + j dil alone) ----
  rg_f32x4 acc[RT][2];
#pragma unroll
  for (int mt = 0; mt < RT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = rg_f32x4{0.f, 0.f, 0.f, 0.f};
  rg_u32x4 af[2][RT][2];
  const unsigned char* const gimg = img + grp * RG * 64;
  auto read_a = [&](auto par_tag, const int c, const int j) {
    constexpr int par = decltype(par_tag)::value;
    const int lrow = r16 + j * p.dil;
    const unsigned char* const a = gimg + c * CS + lrow * 64 + afrag_slot(lrow, kq);
    afrag_read<RT>(af[par], a, PS);
  };
  int nc = 1, nj = 0;      // chunk and tap of the NEXT step
  read_a(std::integral_constant<int, 0>{}, 0, 0);
  auto step = [&](auto par_tag, const bool last) {      // hc_step at NB = 2: buffer = parity
    constexpr int par = decltype(par_tag)::value;
    hc_step<NCH, par, par>(acc, af, bq, w, KS, nc, nj, last, read_a);
  };
#pragma unroll 1
  for (int ks = 0; ks < KS; ks += 2) {
    step(std::integral_constant<int, 0>{}, false);
    step(std::integral_constant<int, 1>{}, ks + 2 >= KS);
  }

  // ---- epilogue, per wave (no workgroup barrier): every row m < M, both residuals optional ----
  hc_epilogue<C, false>(HcStore{p.M, p.out, p.res1, p.res2, p.out_scale, p.accumulate, p.amax_out}, acc, (hc_lds_f32*)patch,
                        (const hc_lds_i32x2*)rowinfo, grp * RG, 0, m0, cs4, b4, ncol, lane);
  // the wrapped-around W loads of the last two steps: bq stays reserved until they have landed (WFragBuf, rule c)
  wait_vmcnt<0>();
  bq.landed_all();
}

}  // namespace jv
