// The shared passes of the vocoder's two row-owning kernels (hiftconv_kernel.h, hiftpair_kernel.h), in ONE place.
// hiftpair_kernel is hiftconv_kernel with an intermediate pass and a second product in the middle; what the two do around and
// inside their products was the same text twice and lives here:
//   * hc_lds_layout    the LDS carve-up, for the kernels' pointers AND the host's byte count (one description, not two);
//   * HcWeights        the walker over the fragment-order weight stream (pointer set-up, load of a step's column block, advance
//                      with the wrap to step 0);
//   * hc_slot_of       a row's utterance slot, by table or by (G, S, nb), clamped;
//   * hc_stage_window  the window pass: four rows in flight, zero-page select, Snake, scale, plane split, keyed LDS stores;
//   * hc_step          a 32-deep step: MFMAs of column block 0, counted wait, next A read, column block 1, advance -- with the
//                      derivation of the wait count;
//   * hc_epilogue      the per-wave epilogue through the 16 x 36 patch with the measured-bound tracking, a tile ahead.
// The kernels are schedules over these pieces.  Unlike row_tail.h's and row_mainloop.h's pieces these OWN their loads, stores
// and LDS addresses: the call sites were two copies of one text, not kernels that chose different orders, and each piece was
// kept only where the built kernels kept their footprint, main loop and load / wait / barrier counts against the written-out
// code (profiles/hift_common_isa.md, which also has the shapes that did not: pass scalars BY VALUE and LDS pointers TYPED as LDS).
// What stays written out in the kernels, deliberately:
//   * the per-row facts pass (the pair has the intermediate's scale and mask: different in substance) and its mask reads;
//   * the pair's intermediate pass, its Snake included (a helper there re-shapes that pass's branches: ~90 instructions);
//   * the prologue's weight requests, as a counted loop (the report has why), WFragBuf's rules (a)-(c), bq.zero() and every
//     vmcnt(0) + landed_all(): the place of each counted wait and barrier stays visible in the kernel text;
//   * read_a, the products' loop structure (rolled in hiftconv_kernel, straight-line in hiftpair_kernel) and JV_HP_WBUF.
#pragma once
#include "rowgemm_kernel.h"

namespace jv {

__device__ __attribute__((aligned(64))) const float hc_zero_page[16] = {};
__device__ __attribute__((aligned(16))) const unsigned char hc_ones_page[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

__device__ __forceinline__ void hc_atomic_max(float* slot, unsigned v) {      // integer max of the bit pattern of a non-negative float
  __hip_atomic_fetch_max((__attribute__((address_space(1))) unsigned*)slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS pointers, said in the type: a helper is optimised on its own before it is inlined, and until then a plain pointer is a
// flat one -- 64-bit address arithmetic, and another pairing of the patch stores (profiles/hift_common_isa.md)
typedef __attribute__((address_space(3))) float hc_lds_f32;
typedef int hc_i32x2 __attribute__((ext_vector_type(2)));      // (int2 is a class on the host pass: no copy out of an address space)
typedef __attribute__((address_space(3))) hc_i32x2 hc_lds_i32x2;
typedef __attribute__((address_space(3))) unsigned char hc_lds_u8;
constexpr int HC_RT = 5, HC_RG = 16 * HC_RT;      // rows per wave (row group)
constexpr int HC_RI_TRACK = 1 << 30;              // rowinfo[].y: the row's utterance slot | this flag when what is stored is tracked

// ---- the LDS carve-up, ONCE: the kernels take their pointers from it, the host the byte count it asks the launch for ----
// window rows, padded: a multiple of 8 plus 1 (an ODD row count puts consecutive chunks 64 bytes apart modulo the 256-byte
// bank row instead of on top of each other -- the staging stores of a wave span two to eight chunks)
__host__ __device__ inline int hc_wrpad(int R, int ntaps, int dil) { return ((R + (ntaps - 1) * dil + 7) & ~7) + 1; }
struct HcLds {      // byte offsets from the start of dynamic LDS
  int yinv1, ysc2;      // wscale float [window rows] is at 0; hiftpair_kernel: float [R] each, the intermediate rows' 1 / scale1 and scale2
  int rowinfo;          // int2 [R]: the output rows' (bits of 1 / scale, slot | HC_RI_TRACK)
  int img;              // [C / 32][2][image rows][64 B]: the operand image (the pair's intermediate is laid over the window)
  int patch;            // float [waves][16][36]: the epilogue's transposition patches
  int total;
};
template <int C, int NG, bool PAIR>
__host__ __device__ inline HcLds hc_lds_layout(const int ntaps, const int dil) {
  constexpr int R = HC_RG * NG, NCH = C / 32;
  const int w1 = hc_wrpad(R, ntaps, dil), w2 = PAIR ? hc_wrpad(R, ntaps, 1) : 0;
  const int wr = PAIR && w2 > w1 ? w2 : w1;      // image rows
  HcLds l;
  l.yinv1 = (w1 * 4 + 255) & ~255;
  l.ysc2 = l.yinv1 + (PAIR ? R * 4 : 0);
  l.rowinfo = l.ysc2 + (PAIR ? R * 4 : 0);
  l.img = l.rowinfo + R * 8;
  l.patch = l.img + NCH * 2 * wr * 64;
  l.total = l.patch + NG * NCH * 16 * 36 * 4;
  return l;
}

// ---- the weight stream: fragment order, [plane][KS][C / 16 blocks][64 lanes][8 halves] (k-step major); the wave of 32-column
// pair cp takes column blocks 2 cp + nt.  The walker and the register buffer it fills (WFragBuf, row_mainloop.h: NB steps of
// lookahead); the counted waits and bq.landed_*() behind them stay in the kernels ----
template <int C>
struct HcWeights {
  const unsigned short* wp[2][2];      // [column block nt][plane]: the next step to request
  int wk;                              // its number
  __device__ __forceinline__ void start(const unsigned short* const Wf, const long wf_plane, const int cp, const int lane) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) wp[nt][pl] = Wf + (long)pl * wf_plane + (long)(2 * cp + nt) * 512 + lane * 8;
    wk = 0;
  }
  template <int buf, int nt, int NB>
  __device__ __forceinline__ void load(WFragBuf<NB>& bq) {
    bq.template load<buf, nt, 0>(wp[nt][0]);
    bq.template load<buf, nt, 1>(wp[nt][1]);
  }
  // + C / 16 blocks x 1 KB (512 halves) per step; past the end: back to the first step (weights that exist: WFragBuf, rule c)
  __device__ __forceinline__ void advance(const int KS) {
    constexpr long WSTEP = 512L * (C / 16);
    const long d = ++wk == KS ? WSTEP - WSTEP * KS : WSTEP;
    if (wk == KS) wk = 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) wp[nt][pl] += d;
  }
};

// ---- one 32-deep step of a product: the A fragments of parity `par` (requested by the step before) times weight buffer `buf`,
// which is refilled for the step NB ahead; behind the first column block the counted wait, then the next step's A fragments
// (read_a(parity, chunk, tap): the kernel's, it knows the image) unless this step is the product's last.
// The wait.  This wave's memory operations in program order: ... W0(s+NB-1), W1(s+NB-1) | W0(s+NB), <wait>, W1(s+NB) | ...;
// needed at the wait: W0(s+1) and W1(s); behind W0(s+1): W1(s+1) .. W0(s+NB) = 2 (NB - 1) load pairs = HC_NWL (NB - 1) loads
// (NB = 2, hiftconv_kernel: W1(s+1) and W0(s+2), rowgemm_wa_kernel's count) ----
constexpr int HC_NWL = 4;
template <int NCH, int buf, int par, int NB, int C, class ReadA>
__device__ __forceinline__ void hc_step(rg_f32x4 (&acc)[HC_RT][2], const rg_u32x4 (&af)[2][HC_RT][2], WFragBuf<NB>& bq, HcWeights<C>& w,
                                        const int KS, int& nc, int& nj, const bool last, const ReadA read_a) {
  auto block = [&](auto nttag) {
    constexpr int nt = decltype(nttag)::value;
#pragma unroll
    for (int mt = 0; mt < HC_RT; ++mt) {
      acc[mt][nt] = h3_mma(acc[mt][nt], af[par][mt][0], af[par][mt][1], bq.q[buf][nt][0], bq.q[buf][nt][1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    w.template load<buf, nt>(bq);
    __builtin_amdgcn_sched_barrier(0);
  };
  block(std::integral_constant<int, 0>{});
  wait_vmcnt<HC_NWL * (NB - 1)>();
  bq.template landed_mid<buf>();
  if (!last) read_a(std::integral_constant<int, par ^ 1>{}, nc, nj);
  __builtin_amdgcn_sched_barrier(0);
  block(std::integral_constant<int, 1>{});
  w.advance(KS);
  if (++nc == NCH) { nc = 0; ++nj; }      // chunk and tap of the NEXT step
}

// ---- a row's utterance slot: by table (the compact geometry of ragged batches, hift.hip; every caller clamps `row` to the
// buffer) or (row - slot_G) / slot_S, clamped to the slots that exist ----
template <class Args>
__device__ __forceinline__ int hc_slot_of(const Args& p, const long row) {
  if (p.slot_map) {
    const int q = p.slot_map[row];
    return q < 0 ? 0 : (q >= p.slot_nb ? p.slot_nb - 1 : q);
  }
  if (p.slot_S <= 0) return 0;
  const int q = (int)((row - p.slot_G) / p.slot_S);
  return q < 0 ? 0 : (q >= p.slot_nb ? p.slot_nb - 1 : q);
}

// ---- the window, once: fp32 rows -> Snake -> x scale -> two fp16 planes, chunk-major operand image [C / 32][2][PS / 64 rows][64 B] ----
// a0: the window's first row in the [rows, C] buffer; wscale[r]: window row r's scale, < 0 = the row reads as zero; NT threads
#ifndef JV_HC_U
#define JV_HC_U 4
#endif
template <int C, int NT>
__device__ __forceinline__ void hc_stage_window(const float* const a0, const int WR, const hc_lds_f32* const wscale, const float* const alpha,
                                                hc_lds_u8* const img, const int CS, const int PS, const int tid) {
  constexpr int C4 = C / 4;                     // float4 per row
  constexpr int RPI = NT / C4;                  // window rows staged per pass of the workgroup
  const int c4 = tid % C4, r0 = tid / C4;      // this thread's four channels, its first window row
  const rg_f32x4 al = *reinterpret_cast<const rg_f32x4*>(alpha + 4 * c4);
  rg_f32x4 ai;
#pragma unroll
  for (int e = 0; e < 4; ++e) ai[e] = 1.0f / (al[e] + 1e-9f);
  const int chunk = c4 >> 3, cslot = (c4 & 7) >> 1, chalf = (c4 & 1) << 3;
  const float* const abase = a0 + 4 * c4;
  // four rows in flight per thread and pass.  (All 12 - 17 of a thread's rows at once measured SLOWER on the same box: the
  // vocoder stage 32.2 ms against 24.6 -- the loop below is then one 8 000-line unrolled body, and two co-resident workgroups
  // hide each other's latency anyway.)
  constexpr int U = JV_HC_U;
  for (int rb = r0; rb < WR; rb += U * RPI) {
    rg_f32x4 x[U];
    float sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rb + u * RPI;
      sc[u] = r < WR ? wscale[r] : -1.f;
      // (explicitly GLOBAL loads; a row that reads as zero is fetched from a page of zeros and never multiplied: guard rows
      // may hold anything)
      const float* src = sc[u] >= 0.f ? abase + (long)r * C : hc_zero_page;
      x[u] = *(const __attribute__((address_space(1))) rg_f32x4*)src;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rb + u * RPI;
      if (r >= WR) continue;
      rg_f32x4 v = x[u];
      if (sc[u] >= 0.f) {
        float arg[4];
        bool big = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          arg[e] = v[e] * al[e];
          big = big || fabsf(arg[e]) > 32768.f;      // false for NaN, which sin2_small propagates
        }
        if (snake_args_small(big)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] + ai[e] * sin2_small(arg[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float sn = sinf(arg[e]);
            v[e] = v[e] + ai[e] * (sn * sn);
          }
        }
        v = v * sc[u];
      } else {
        v = rg_f32x4{0.f, 0.f, 0.f, 0.f};
      }
      const Split2 s0 = split2h_pair(v[0], v[1]);
      const Split2 s1 = split2h_pair(v[2], v[3]);
      hc_lds_u8* d = img + chunk * CS + r * 64 + (((cslot ^ rg_key(r))) << 4) + chalf;
      *(__attribute__((address_space(3))) rg_u32x2*)d = rg_u32x2{s0.h, s1.h};
      *(__attribute__((address_space(3))) rg_u32x2*)(d + PS) = rg_u32x2{s0.l, s1.l};
    }
  }
}

// ---- epilogue, per wave (no workgroup barrier): 16 rows at a time through the wave's private 16 x 36-float patch (MFMA
// layout in: lane = column, 4 rows; rows out: 8 lanes x 16 B per row), so that every store writes whole 128-byte row segments:
//   out = ((acc * inv * cs4 + b4) + res1 + res2) * out_scale (+ previous out),   max |out| of the tracked rows into amax_out.
// rowb: the wave's first tile row; rowinfo[tile row] = (bits of 1 / the row's staging scale, slot | HC_RI_TRACK); ncol: the
// lane's four columns.  PAIR (hiftpair_kernel): only tile rows < RO are output rows, and res1 (the block's input) is never
// null; hiftconv_kernel stores every row m < M and has no RO.
struct HcStore {      // the fields of the kernels' argument structs the epilogue reads, by value
  int M;
  float* out;
  const float *res1, *res2;
  float out_scale;
  int accumulate;
  float* amax_out;
};
template <int C, bool PAIR>
__device__ __forceinline__ void hc_epilogue(const HcStore p, const rg_f32x4 (&acc)[HC_RT][2], hc_lds_f32* const patch, const hc_lds_i32x2* const rowinfo,
                                            const int rowb, const int RO, const int m0, const rg_f32x4 cs4, const rg_f32x4 b4,
                                            const int ncol, const int lane) {
  const float* const res1 = p.res1;
  constexpr int RT = HC_RT, RI_TRACK = HC_RI_TRACK;
  const int r16 = lane & 15, kq = lane >> 4;
  const int prow = lane >> 3;
  const float* const r1b = PAIR || res1 ? res1 + ncol : nullptr;
  const float* const r2b = p.res2 ? p.res2 + ncol : nullptr;
  float* const ob = p.out + ncol;
  struct RowIn { rg_f32x4 r1[2], r2[2], pv[2]; float inv[2]; int info[2]; bool ok[2]; };
  auto request = [&](const int mt, RowIn& in) {      // the two 8-row halves of row tile mt
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int trow = rowb + mt * 16 + ps * 8 + prow;
      const long m = (long)m0 + trow;
      long mc;
      if constexpr (PAIR) {
        in.ok[ps] = trow < RO && m < p.M;
        mc = in.ok[ps] ? m : (m < p.M ? m : (long)p.M - 1);
      } else {
        in.ok[ps] = m < p.M;
        mc = in.ok[ps] ? m : (long)p.M - 1;
      }
      const hc_i32x2 ri = rowinfo[trow];
      in.inv[ps] = __uint_as_float((unsigned)ri.x);
      in.info[ps] = ri.y;
      const rg_f32x4 z = {0.f, 0.f, 0.f, 0.f};
      // (explicitly GLOBAL, like every load and store here: a flat access counts on lgkmcnt too and would sit in every LDS wait)
      if constexpr (PAIR) in.r1[ps] = *(const __attribute__((address_space(1))) rg_f32x4*)(r1b + mc * C);
      else in.r1[ps] = r1b ? *(const __attribute__((address_space(1))) rg_f32x4*)(r1b + mc * C) : z;
      in.r2[ps] = r2b ? *(const __attribute__((address_space(1))) rg_f32x4*)(r2b + mc * C) : z;
      in.pv[ps] = p.accumulate ? *(const __attribute__((address_space(1))) rg_f32x4*)(ob + mc * C) : z;
    }
  };
  auto finish = [&](const int mt, const RowIn& in) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) patch[(kq * 4 + e) * 36 + nt * 16 + r16] = acc[mt][nt][e];
    unsigned u = 0u;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int trow = rowb + mt * 16 + ps * 8 + prow;
      const long m = (long)m0 + trow;
      rg_f32x4 x = *(const __attribute__((address_space(3))) rg_f32x4*)(patch + (ps * 8 + prow) * 36 + 4 * (lane & 7));
      x = x * in.inv[ps];      // 1 / the power of two the row's utterance was staged with
      rg_f32x4 t = x * cs4 + b4;
      t = (t + in.r1[ps]) + in.r2[ps];
      const rg_f32x4 res = t * p.out_scale + in.pv[ps];
      if (in.ok[ps]) {
        *(__attribute__((address_space(1))) rg_f32x4*)(ob + m * C) = res;
        if (in.info[ps] & RI_TRACK) {
#pragma unroll
          for (int e = 0; e < 4; ++e) u = max(u, __float_as_uint(res[e]) & 0x7fffffffu);
        }
      }
    }
    if (p.amax_out) {
      // the 16 rows of a tile almost always belong to one utterance: one wave-level maximum, one atomic -- and none once the
      // slot already holds a larger value (a plain, cacheable read of it: a slot only grows).  Rows of two utterances: per lane.
      const int s_lo = rowinfo[rowb + mt * 16].y & (RI_TRACK - 1), s_hi = rowinfo[rowb + mt * 16 + 15].y & (RI_TRACK - 1);
      if (s_lo == s_hi) {
        const unsigned seen = *(const __attribute__((address_space(1))) unsigned*)(p.amax_out + s_lo);
        if (__builtin_amdgcn_ballot_w64(u > seen) != 0) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, o));
          if (lane == 0) hc_atomic_max(p.amax_out + s_lo, u);
        }
      } else {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
          unsigned v = 0u;
          const int trow = rowb + mt * 16 + ps * 8 + prow;
          const long m = (long)m0 + trow;
          if (in.ok[ps] && (in.info[ps] & RI_TRACK)) {
            const rg_f32x4 res = *(const __attribute__((address_space(1))) rg_f32x4*)(ob + m * C);      // (this lane's own store)
#pragma unroll
            for (int e = 0; e < 4; ++e) v = max(v, __float_as_uint(res[e]) & 0x7fffffffu);
            hc_atomic_max(p.amax_out + (in.info[ps] & (RI_TRACK - 1)), v);
          }
        }
      }
    }
  };
  RowIn cur, nxt;
  request(0, cur);
#pragma unroll
  for (int mt = 0; mt < RT; ++mt) {
    if (mt + 1 < RT) request(mt + 1, nxt);      // a tile ahead: its loads travel while this one is finished
    finish(mt, cur);
    cur = nxt;
  }
}

}  // namespace jv
