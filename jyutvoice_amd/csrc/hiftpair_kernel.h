// One launch for a ResBlock's convolution PAIR in the vocoder (jyutvoice/hifigan/generator.py:90-97):
//   xt = Conv1d(C, C, k, dilation d)(Snake1(x));  xt = Conv1d(C, C, k)(Snake2(xt));  x = xt + x
// at C = 64 / 128 channels (the 120 T + 1 and 40 T rows per utterance: 1.15 M / 384 K rows at the benchmarked size).
//
// Why.  As two hiftconv_kernel launches the pair moves five tensors -- x in, xt out, xt in, x in again as the residual, the
// result out -- for 2 k C^2 multiply-adds per element: at C = 64 that is 0.86 GB per launch for 28 GFLOP x k, and the launch
// takes 360 us where its MFMAs need 42 / 97 / 153 us (k = 3 / 7 / 11, fp16x3 at the clock the chip holds) and its bytes ~150:
// load, Snake, MFMAs and stores of a workgroup run one after the other and two co-resident workgroups overlap them only in
// part.  Here the intermediate never leaves LDS: three tensor passes instead of five, one prologue and one epilogue per pair.
//
// A workgroup (hiftconv_kernel's shape: NG C / 32 waves, each a 80 x 32 tile of both products) owns R = 80 NG rows of the
// INTERMEDIATE, i.e. RO = R - (k - 1) output rows (the second convolution's halo is recomputed by the neighbours: 2 - 7 % of
// the first product):
//   1. the window of x -- R + (k - 1) d rows -- through Snake1 and the plane split into LDS, once (hiftconv_kernel's pass);
//   2. first product: intermediate rows m0 - h2 .. m0 - h2 + R - 1 (h2 = (k - 1) / 2), accumulators in registers;
//   3. the accumulators -> + bias -> mask (rows outside the utterance's frames read as ZERO in the second convolution: its
//      "same" padding) -> Snake2 -> x scale2 -> planes, written over the window's image in the operand layout (rowblock_kernel's
//      GELU pass: neighbouring lanes trade one row of each pair and store whole dwords);
//   4. second product (dilation 1) over that image: output rows m0 .. m0 + RO - 1 are tile rows 0 .. RO - 1;
//   5. per-wave epilogue: + bias + x (re-read: 41 KB per workgroup, L2-warm) (+ a second residual), scaling, accumulation,
//      measured-bound tracking of what is stored -- hiftconv_kernel's.
// The weights of both convolutions arrive as ONE fragment stream (k-step major fragments: the second's steps follow the first's,
// registry.hip) through the register double buffer with hand-counted waits (WFragBuf's rules: row_mainloop.h; tools/check_rowgemm_isa.py).
//
// The intermediate's fp16x3 scale.  Unfused, the first launch MEASURES max |xt| per utterance and the second derives its power
// of two from it.  Here no such maximum exists before the intermediate is consumed, so the scale comes from a BOUND instead:
//   |xt| <= L1 (amax_x + e1) + max |b1|,   L1 = the largest row L1 norm of the first convolution's weights (load time),
// amax_x the measured bound of x of the row's utterance, e1 / e2 what Snake1 / Snake2 can add (max 1 / alpha).  Overflow is
// impossible by construction as before; the bound is looser than a measurement (typically 5 - 20 x), which costs nothing in
// relative precision (22 bits per element down to 2^-17 of the bound) and moves the absolute floor (2^-40 of the bound) by
// as much.  A function of the utterance alone: results do not depend on the batch or on where a row sits.  Fused and unfused
// agree to rounding: both sit inside the same fp64 bound (tests/test_gpu_fused_ops.py::test_hiftpair_against_two_hiftconv_launches;
// end to end: tests/test_gpu_pipeline.py).
#pragma once
#include "hiftconv_kernel.h"

namespace jv {

struct HiftPairArgs {
  const float* A;                  // the block's input x, fp32 rows [rows, C]; also the residual
  long a_rows;                     // rows of A that may be read (others read as zero)
  int M;                           // output rows
  int ntaps, dil;                  // k (both convolutions), the first one's dilation; "same" padding on both
  const unsigned char* rowmask;    // per row or null: 0 -> the row reads as zero, as x and as the intermediate; not tracked
  const float *alpha1, *alpha2;    // Snake parameters per channel
  const unsigned short* Wf;        // fragment order over K = 2 k C: the first convolution's k C / 32 steps, then the second's
  long wf_plane;
  const float *cs1, *b1, *cs2, *b2;      // column scales (2^-e_n) and biases of the two convolutions
  const float* amax_in;            // per-utterance measured bound of x
  float e1, e2;                    // max 1 / (alpha + 1e-9) of Snake1 / Snake2
  float l1max, b1max;              // largest row L1 norm and largest |bias| of the first convolution
  int slot_G, slot_S, slot_nb;     // slot(row) = clamp((row - slot_G) / slot_S, 0, slot_nb - 1)
  const int* slot_map;             // or, when set: slot(row) = slot_map[row] (HiftConvArgs::slot_map)
  float* out;                      // [rows, C]: out = ((acc2 + b2) + x + res2) * out_scale (+ previous out)
  const float* res2;               // [rows, C] or null
  float out_scale;
  int accumulate;
  float* amax_out;                 // tracking of what is stored, per utterance slot (rows with rowmask == 0 excluded)
  long alg_rows;
};

template <int NG> constexpr int hp_rows() { return HC_RG * NG; }
template <int C, int NG> inline int hp_lds_bytes(int ntaps, int dil) { return hc_lds_layout<C, NG, true>(ntaps, dil).total; }

template <int N, class F, int... Is>
__device__ __forceinline__ void hp_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void hp_for(F&& f) {
  hp_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}

// KT: the kernel size, a template parameter -- the step sequence of both products is then straight-line code, every step's
// weight buffer (step mod NB) and A-fragment parity (step mod 2) a compile-time constant.  (Chosen at run time through a
// switch per step, the six (buffer, parity) combinations made the register allocator copy the buffers at every join: 567
// spilled registers, and copies of registers with loads in flight are exactly what tools/check_rowgemm_isa.py forbids.)
template <int C, int NG, int KT>
__global__ __launch_bounds__(64 * NG * (C / 32), 2) void hiftpair_kernel(const HiftPairArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hc_lds[];
  constexpr int RT = HC_RT, RG = HC_RG;
  constexpr int NCH = C / 32, CW = C / 32, R = RG * NG, NT = 64 * NG * CW;
  static_assert(R + 56 <= NT, "one window row per thread in the facts pass");
  typedef const __attribute__((address_space(1))) unsigned char* gbytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int grp = wave / CW, cp = wave % CW;    // row group, 32-column pair
  constexpr int k = KT;
  const int h2 = (k - 1) >> 1, h1 = (p.dil * (k - 1)) >> 1;
  const int RO = R - (k - 1);                   // output rows of this workgroup
  const int m0 = blockIdx.x * RO;
  const int WR = R + (k - 1) * p.dil;           // window rows of x really used
  const int WRP = ((WR + 7) & ~7) + 1;
  const int WRP2 = ((R + (k - 1) + 7) & ~7) + 1;      // rows of the intermediate's image (its last k - 1 are never written: they
                                                      // reach discarded output rows only)
  const int PS = WRP * 64, CS = 2 * PS;         // plane and chunk strides of the window's image
  const int PS2 = WRP2 * 64, CS2 = 2 * PS2;     // ... and of the intermediate's, laid over it
  constexpr int KS1 = k * NCH;                  // 32-deep steps per convolution (even: NCH is)
  constexpr int KS = 2 * KS1;
  const HcLds L = hc_lds_layout<C, NG, true>(k, p.dil);
  float* const wscale = reinterpret_cast<float*>(hc_lds);                                   // [WRP]: < 0 = the row reads as zero
  float* const yinv1 = reinterpret_cast<float*>(hc_lds + L.yinv1);                          // [R]: 1 / scale1 of the intermediate row's utterance
  float* const ysc2 = reinterpret_cast<float*>(hc_lds + L.ysc2);                            // [R]: scale2 of it; < 0 = the row reads as zero
  int2* const rowinfo = reinterpret_cast<int2*>(hc_lds + L.rowinfo);                        // [R]: output rows (x = bits of 1 / scale2)
  unsigned char* const img = hc_lds + L.img;                                                // [NCH][2][max(WRP, WRP2)][64 B]
  float* const patch = reinterpret_cast<float*>(hc_lds + L.patch) + wave * (16 * 36);

  // ---- W: this wave's fragment stream of BOTH convolutions through the register buffers; steps 0 .. NB - 1 are requested here ----
  // NB weight buffers: a step's fragments are requested NB steps ahead.  Two (the trunk kernels' double buffer) is 1.5 steps
  // of lookahead at the first wait -- at ONE wave per SIMD and workgroup, as here, less than an L2 round trip (rowblock's
  // staggered schedule measured it: 930 cycles per step for a lone wave against 480 of MFMA issue); this kernel has the 16
  // registers a third buffer costs.
#ifndef JV_HP_WBUF
#define JV_HP_WBUF 3
#endif
  constexpr int NB = JV_HP_WBUF;
  static_assert(NB == 2 || NB == 3, "two or three weight buffers");
  HcWeights<C> w;
  w.start(p.Wf, p.wf_plane, cp, lane);
  WFragBuf<NB> bq;
  bq.zero();
  // the weights start first: everything below is global-load latency they spend in flight.  (A counted loop that the compiler
  // unrolls, on purpose: as straight-line steps, here or in the walker, the same loads leave hiftpair_kernel<128,2,11> with four
  // VGPRs more -- profiles/hift_common_isa.md)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b == 0) { w.template load<0, 0>(bq); w.template load<0, 1>(bq); }
    if (b == 1) { w.template load<1, 0>(bq); w.template load<1, 1>(bq); }
    if (b == 2) { w.template load<NB - 1, 0>(bq); w.template load<NB - 1, 1>(bq); }
    w.advance(KS);
  }

  // ---- per-row facts (one level of unconditional loads on clamped indices: rowconv_wd_kernel).  Written out in both kernels:
  // this one has the intermediate's scale and mask ----
  auto slot_of = [&](const long row) { return hc_slot_of(p, row); };
  constexpr int RI_TRACK = HC_RI_TRACK;
  {
    // window row tid <-> global row m0 - h2 - h1 + tid; intermediate row tid <-> m0 - h2 + tid; output row tid <-> m0 + tid
    const long ar = (long)m0 - h2 - h1 + tid;
    const bool in_w = tid < WR && ar >= 0 && ar < p.a_rows;
    const long arc = ar < 0 ? 0 : (ar < p.a_rows ? ar : p.a_rows - 1);
    const int mk = ((gbytes)(p.rowmask ? p.rowmask : hc_ones_page))[p.rowmask ? arc : 0];
    const float am_w = p.amax_in[slot_of(arc)];
    const long yr = (long)m0 - h2 + (tid < R ? tid : 0);
    const bool in_y = yr >= 0 && yr < p.M;
    const long yrc = yr < 0 ? 0 : (yr < p.M ? yr : (long)p.M - 1);
    const int mky = ((gbytes)(p.rowmask ? p.rowmask : hc_ones_page))[p.rowmask ? yrc : 0];
    const float am_y = p.amax_in[slot_of(yrc)];
    const long mt = (long)m0 + (tid < R ? tid : 0);
    const long mc = mt < p.M ? mt : (long)p.M - 1;
    const int sl_o = slot_of(mc);
    const int trk = ((gbytes)(p.rowmask ? p.rowmask : hc_ones_page))[p.rowmask ? mc : 0];
    const float am_o = p.amax_in[sl_o];
    if (tid < WRP) wscale[tid] = (in_w && mk != 0) ? h3_scale_dev(am_w + p.e1) : -1.f;
    if (tid < R) {
      // the intermediate's scale from its BOUND (header): a function of the utterance's measured bound of x alone
      yinv1[tid] = 1.0f / h3_scale_dev(am_y + p.e1);
      ysc2[tid] = (in_y && mky != 0) ? h3_scale_dev(p.l1max * (am_y + p.e1) + p.b1max + p.e2) : -1.f;
      const bool ok = tid < RO && mt < p.M;
      const float inv = ok ? 1.0f / h3_scale_dev(p.l1max * (am_o + p.e1) + p.b1max + p.e2) : 0.f;
      rowinfo[tid] = int2{(int)__float_as_uint(inv), sl_o | ((p.amax_out && ok && trk != 0) ? RI_TRACK : 0)};
    }
  }
  __syncthreads();

  // ---- the window, once: fp32 rows -> Snake1 -> x scale -> two fp16 planes, chunk-major operand image ----
  hc_stage_window<C, NT>(p.A + ((long)m0 - h2 - h1) * C, WR, (const hc_lds_f32*)wscale, p.alpha1, (hc_lds_u8*)img, CS, PS, tid);
  // per-column constants: this lane's columns in the MFMA layout (the intermediate) and in the row-wise passes (the epilogue)
  float cs1c[2], b1c[2], al2c[2], ai2c[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int col = 32 * cp + 16 * nt + r16;
    cs1c[nt] = p.cs1[col];
    b1c[nt] = p.b1 ? p.b1[col] : 0.f;
    al2c[nt] = p.alpha2[col];
    ai2c[nt] = 1.0f / (al2c[nt] + 1e-9f);
  }
  const int ncol = 32 * cp + 4 * (lane & 7);
  rg_f32x4 cs4 = *reinterpret_cast<const rg_f32x4*>(p.cs2 + ncol);
  rg_f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (p.b2) b4 = *reinterpret_cast<const rg_f32x4*>(p.b2 + ncol);
  wait_vmcnt<0>();
  bq.landed_all();
  lds_barrier();      // the window's image is complete

  // ---- the two products: step ks = (tap j = ks / NCH, chunk c = ks % NCH); A fragments of row tile mt at image row
  // 80 grp + 16 mt + r16 + j dil (the 16-byte slot key depends on r16 + j dil alone) ----
  rg_f32x4 acc[RT][2];
  rg_u32x4 af[2][RT][2];
  int ips = PS, ics = CS, idil = p.dil;      // the image being read: plane / chunk strides, row step per tap
  auto read_a = [&](auto par_tag, const int c, const int j) {
    constexpr int par = decltype(par_tag)::value;
    const int lrow = r16 + j * idil;
    const unsigned char* const a = img + grp * RG * 64 + c * ics + lrow * 64 + afrag_slot(lrow, kq);
    afrag_read<RT>(af[par], a, ips);
  };
  int nc = 1, nj = 0;      // chunk and tap of the NEXT step
  auto step = [&](auto buf_tag, auto par_tag, const bool last) {
    hc_step<NCH, decltype(buf_tag)::value, decltype(par_tag)::value>(acc, af, bq, w, KS, nc, nj, last, read_a);
  };
  // product P0 / KS1 (P0 = its first step's number over both products): weight buffer (P0 + i) % NB, A parity i & 1 (KS1 is even)
  auto product = [&](auto p0_tag) {
    constexpr int P0 = decltype(p0_tag)::value;
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = rg_f32x4{0.f, 0.f, 0.f, 0.f};
    nc = 1; nj = 0;
    read_a(std::integral_constant<int, 0>{}, 0, 0);
    hp_for<KS1>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      step(std::integral_constant<int, (P0 + i) % NB>{}, std::integral_constant<int, i & 1>{}, i + 1 >= KS1);
    });
  };
  product(std::integral_constant<int, 0>{});      // the intermediate, before its bias, x scale1 x 2^e

  // ---- the intermediate: + bias -> mask -> Snake2 -> x scale2 -> planes, over the window's image ----
  lds_barrier();      // every wave is done reading the window
  {
    unsigned char* const hs = img + cp * CS2 + grp * RG * 64;      // this wave's 32 channels are chunk cp, its rows group grp
    const int key = (kq & 1) << 1;      // rg_key of image row 80 grp + 16 mt + 4 kq + e (bit 2 of it is bit 0 of kq)
    const int odd = r16 & 1;
    // v_perm_b32 selectors (rowblock_kernel.h's GELU pass): even lane: (mine.lo16 | partner.lo16 << 16), odd: (partner.hi16 | mine.hi16 << 16)
    const unsigned sel = odd ? 0x03020706u : 0x05040100u;
#pragma unroll
    for (int mt = 0; mt < RT; ++mt) {
      const int i0 = grp * RG + mt * 16 + kq * 4;      // this lane's four intermediate rows
      const rg_f32x4 inv4 = *reinterpret_cast<const rg_f32x4*>(yinv1 + i0);
      const rg_f32x4 sc4 = *reinterpret_cast<const rg_f32x4*>(ysc2 + i0);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int slot = (2 * nt + (r16 >> 3)) ^ key;
        // (Snake as in hc_stage_window, hift_common.h, per column and with the masked rows out of the range test; written out: a
        // shared helper re-shapes this pass's branches, profiles/hift_common_isa.md)
        float g4[4], arg[4];
        bool big = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          g4[e] = acc[mt][nt][e] * (cs1c[nt] * inv4[e]) + b1c[nt];
          arg[e] = g4[e] * al2c[nt];
          big = big || (sc4[e] >= 0.f && fabsf(arg[e]) > 32768.f);
        }
        if (snake_args_small(big)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) g4[e] = g4[e] + ai2c[nt] * sin2_small(arg[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float sn = sinf(arg[e]);
            g4[e] = g4[e] + ai2c[nt] * (sn * sn);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) g4[e] = sc4[e] >= 0.f ? g4[e] * sc4[e] : 0.f;      // (selected, never multiplied)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const Split2 sp = split2h_pair(g4[e], g4[e + 1]);      // (row e | row e + 1 << 16) of this lane's column
          const unsigned ph = (unsigned)__builtin_amdgcn_update_dpp(0, (int)sp.h, 0xB1, 0xf, 0xf, true);      // the neighbour's
          const unsigned pl = (unsigned)__builtin_amdgcn_update_dpp(0, (int)sp.l, 0xB1, 0xf, 0xf, true);
          const unsigned wh = __builtin_amdgcn_perm(ph, sp.h, sel), wl = __builtin_amdgcn_perm(pl, sp.l, sel);
          const int row = mt * 16 + kq * 4 + e + odd;
          unsigned char* d = hs + row * 64 + (slot << 4) + (r16 & 6) * 2;
          *reinterpret_cast<unsigned*>(d) = wh;
          *reinterpret_cast<unsigned*>(d + PS2) = wl;
        }
      }
    }
  }
  lds_barrier();      // the intermediate's image is complete
  ips = PS2; ics = CS2; idil = 1;
  product(std::integral_constant<int, KS1>{});

  // ---- epilogue, per wave: out = ((acc + b2) + x + res2) * out_scale (+ previous out) for tile rows < RO (x re-read as res1) ----
  hc_epilogue<C, true>(HcStore{p.M, p.out, p.A, p.res2, p.out_scale, p.accumulate, p.amax_out}, acc, (hc_lds_f32*)patch,
                       (const hc_lds_i32x2*)rowinfo, grp * RG, RO, m0, cs4, b4, ncol, lane);
  // the wrapped-around W loads of the last two steps: bq stays reserved until they have landed (WFragBuf, rule c)
  wait_vmcnt<0>();
  bq.landed_all();
}

}  // namespace jv
