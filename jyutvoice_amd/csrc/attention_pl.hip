// fp16x3 self-attention of the estimator with K and V arriving PRE-SPLIT (two fp16 planes each, written once by the qkv
// GEMM's epilogue) -- jyutvoice/flow/transformer.py:380-389 -> diffusers AttnProcessor2_0 as restated in oracle/flow.py:46-58.
//
// attn64_x6_kernel (attention.hip) stages K / V through registers and splits them into planes in every one of a head's
// query-tile workgroups: round 1's PMC had its vector pipe 49 % busy against 25 % for the matrix pipe, a quarter of the
// vector instructions being that staging.  Here:
//   * K / V tiles of 32 keys go global -> LDS by LDS-DMA (global_load_lds_dwordx4, 16 one-KiB pieces per tile) into a
//     3-stage ring: counted s_waitcnt vmcnt, one bare s_barrier per key tile, two tiles in flight -- no staging VALU, no
//     staging registers, no ds_write;
//   * V stays row-major [key][d] in LDS (what the DMA can deliver) and the PV product's A operand, 8 consecutive keys of
//     one d, is read with gfx950's transposing ds_read_b64_tr_b16 (tools/probes/ds_read_tr16.hip): the 4-key blocks it
//     returns are exactly the key order the S^T accumulator already has (register e of lane-half h holds key
//     (e & 3) + 8 (e >> 2) + 4 h), so P still goes from the softmax to the MFMA with conversions only;
//   * the result leaves as the output projection's pre-split operand (fp16 planes) through LDS, as whole 128-byte rows.
// Arithmetic (scales, base-2 softmax on raw v_exp_f32, products hh' + hl' + lh', smallest first): attention_common.h's pieces, the
// ones attention.hip's NP = 2 path and attention_s.hip call -- term for term the same.
#include <math.h>
#include <stdlib.h>

#include "attention_common.h"

namespace jv {

namespace {

constexpr int PL_NSTAGE = 3;

template <int NW, int NST, int NP = 3>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : (NST == 2 ? 4 : 3)) void attn64_pl_kernel(const AttnArgs p) {
  // the ring, reused at the end for the [2 planes][32 NW queries][128 B] output image
  constexpr int LDS_BYTES = NST * KV_STAGE > 2 * 32 * NW * 128 ? NST * KV_STAGE : 2 * 32 * NW * 128;
  __shared__ __attribute__((aligned(256))) unsigned char lds[LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, half = lane >> 5;
  int b, h, qt;
  {
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int nqt = (p.L + 32 * NW - 1) / (32 * NW);
    // (Tried: a head's partial workgroup -- 44 of 128 queries at 300 frames -- scheduled behind ALL full ones instead of behind its
    // own head's: 36.9 against 34.3 ms per pass on the same box.  The interleaved order lets the short workgroups free slots
    // throughout the launch; at the end they leave the chip a quarter full.)
    qt = lid % nqt;
    h = (lid / nqt) % p.H;
    b = lid / (nqt * p.H);
  }
  const int q0 = qt * 32 * NW + wave * 32;
  // AttnGeo's three lines (attention_common.h), written out: as a helper, in any of four shapes, they change this kernel's prologue
  const int len = p.lens ? min(p.lens[b], p.L) : p.L;
  const long rowbase = p.uoff ? (long)p.uoff[b] : (long)p.G + (long)b * p.S;
  const int Lq = p.uoff ? len : p.L;
  if (qt * 32 * NW >= Lq) return;      // (the whole workgroup: nothing of it lies inside the utterance; uniform geometry: never)
  const bool active = q0 < Lq;

  // Q planes: lane (query, half) holds d = 16 s + 8 half + j for k-step s, pre-scaled by log2(e) / 8 * q_scale
  u32x4 q[4][2];
  const float qsc = q_prescale(p.q_scale);
  const float sinv = 1.0f / (p.q_scale * p.k_scale);      // powers of two: exact
  {
    const int qi = q0 + r32;
    const float* src = p.qkv + (rowbase + qi) * p.ld + h * 64 + 8 * half;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
      if (qi < Lq) {
        t0 = *reinterpret_cast<const f32x4*>(src + 16 * s);
        t1 = *reinterpret_cast<const f32x4*>(src + 16 * s + 4);
      }
      q_split8(t0, t1, qsc, q[s][0], q[s][1]);
    }
  }

  // ---- this wave's DMA pieces of a key tile (attention_common.h: kv_piece)
  constexpr int PPW = 16 / NW;
  const unsigned short* src[PPW];
  int dst[PPW], krel[PPW];
  const int kstride = p.kv_ld;
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const KvPiece pc = kv_piece(wave + NW * i, lane);
    const int slot = kv_slot<VT_4x64>(pc.opv, pc.krel, lane);
    krel[i] = pc.krel;
    src[i] = p.kv2 + (long)pc.pl * p.kv2_plane + rowbase * kstride + pc.opv * 512 + h * 64 + 8 * slot;
    dst[i] = pc.dst;
  }
  auto issue = [&](int k0, int stage) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) kv_issue_piece(src[i], dst[i], krel[i], kstride, k0, len, lds + stage * KV_STAGE);
  };

  int kend = len, kmax = len;
  if (p.chunk > 0) {      // chunk-causal (streaming) mask: jyutvoice/utils/mask.py:91-126
    kend = min(len, ((q0 + r32) / p.chunk + 1) * p.chunk);
    kmax = min(len, ((qt * 32 * NW + 32 * NW - 1) / p.chunk + 1) * p.chunk);
  }
  const int nkt = (kmax + 31) >> 5;

  f32x16 o0, o1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
  float m_run = -INFINITY, l_run = 0.f;

  if (nkt > 0) issue(0, 0);
  if (NST > 2 && nkt > 1) issue(32, 1);
  // per-lane read offsets
  const int k_off = r32 * 128;                                   // + pl * KV_PLANE + slot
  const int vq = (lane & 15) >> 2, vp = lane & 3, vg = (lane >> 4) & 1;      // transposed read: block row, 8-byte piece, 16-d group
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * 32;
    // NST = 3: tile kt has landed when only tile kt + 1's pieces are outstanding; tile kt + 2 goes into the stage tile kt - 1
    // left.  NST = 2 (32 KB: four workgroups per CU instead of three): nothing else is in flight at the wait, and tile kt + 1
    // is issued behind the barrier into the stage tile kt - 1 left
    if (NST > 2 && kt + 1 < nkt) wait_vmcnt<PPW>(); else wait_vmcnt<0>();
    bare_barrier();
    if (NST > 2) { if (kt + 2 < nkt) issue(k0 + 64, (kt + 2) % NST); }
    else if (kt + 1 < nkt) issue(k0 + 32, (kt + 1) % NST);
    if (!active) continue;
    const unsigned char* const sK = lds + (kt % NST) * KV_STAGE;
    const unsigned char* const sV = sK + 2 * KV_PLANE;
    // S^T[key][query] = sum_d K[key][d] * Q[query][d]
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      u32x4 a[2];
      const int ko = ((2 * st + half) ^ kv_k_swz(r32)) << 4;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) a[pl] = *reinterpret_cast<const u32x4*>(sK + pl * KV_PLANE + k_off + ko);
      s = h3_mma32<NP>(a, q[st], s);
    }
    if (__builtin_amdgcn_ballot_w64(k0 + 32 > kend) != 0) {      // wave-uniform: only tiles that straddle a mask edge
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * half;
        s[e] = key < kend ? s[e] : -INFINITY;
      }
    }
    float mt = s[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(mt, s[e]);
    mt = half_max(mt) * sinv;
    const float m_new = attn_lazy_max(m_run, mt);      // (= max(m_run, mt) up to the margin: jv_device.h)
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float lt = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = __builtin_amdgcn_exp2f(fmaf(s[e], sinv, 10.f - m_new));      // probabilities kept as p * 2^10 (cancels in 1 / l)
      lt += s[e];
    }
    lt = half_sum(lt);
    l_run = l_run * alpha + lt;
    m_run = m_new;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
    }
    // O^T[d][query] += sum_key V[key][d] * P[query][key]
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      u32x4 pb[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const Split2 t = split2h_pair(s[8 * st + 2 * e], s[8 * st + 2 * e + 1]);
        pb[0][e] = t.h;
        pb[1][e] = t.l;
      }
#pragma unroll
      for (int db = 0; db < 2; ++db) {      // d 0..31 -> o0, 32..63 -> o1
        // element j of this lane's fragment is key 16 st + 8 (j >> 2) + 4 half + (j & 3): two 4-key blocks
        u32x4 a[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
          for (int rd = 0; rd < 2; ++rd) {
            const int key = 16 * st + 8 * rd + 4 * half + vq;
            const int byte = (db * 32 + vg * 16 + 4 * vp) * 2;
            const int off = key * 128 + ((((byte >> 4) ^ kv_v_swz<VT_4x64>(key)) << 4) | (byte & 15));      // (vt_off, written out: see there)
            const u32x2 u = vt_read4(sV + pl * KV_PLANE + off);
            a[pl][2 * rd] = u[0];
            a[pl][2 * rd + 1] = u[1];
          }
        }
        if (db == 0) o0 = h3_mma32<NP>(a, pb, o0);
        else o1 = h3_mma32<NP>(a, pb, o1);
      }
    }
  }

  // ---- result: O / l, as the output projection's operand.  Through LDS so that every store instruction writes whole
  // 128-byte rows (from the MFMA layout a lane owns 16-byte pieces of 8 different 2 KB rows per instruction)
  lds_barrier();      // every wave is done with the ring
  const float vsc = p.v_scale;
  const float inv = l_run > 0.f ? (1.0f / vsc) / l_run : 0.f;
  if (p.out2) {
    unsigned char* const so = lds;      // [2 planes][32 NW queries][128 B]
    if (active) {
      const float sc = inv * p.out2_scale;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const f32x16& o = db ? o1 : o0;
          const Split2 a0 = split2h_pair(o[4 * g] * sc, o[4 * g + 1] * sc);
          const Split2 a1 = split2h_pair(o[4 * g + 2] * sc, o[4 * g + 3] * sc);
          // d = 32 db + 8 g + 4 half .. + 3: 8 bytes, half of 16-byte chunk 4 db + g of the row; chunks XOR-keyed by the row
          // (unkeyed the 32 rows of a store meet 16 lanes per bank pair: attention_s.hip, profiles/r03_pmc_bench.md)
          unsigned char* dstp = so + (wave * 32 + r32) * 128 + (((4 * db + g) ^ ((r32 >> 1) & 7)) << 4) + 8 * half;
          *reinterpret_cast<u32x2*>(dstp) = u32x2{a0.h, a1.h};
          *reinterpret_cast<u32x2*>(dstp + 32 * NW * 128) = u32x2{a0.l, a1.l};
        }
      }
    }
    lds_barrier();
    // 8 lanes per row of 128 B; 8 rows per wave-instruction
#pragma unroll
    for (int it = 0; it < (2 * 32 * NW * 8) / (64 * NW); ++it) {
      const int idx = it * 64 * NW + tid;
      const int pl = idx / (32 * NW * 8), rem = idx % (32 * NW * 8);
      const int qrow = rem >> 3, piece = rem & 7;
      const int qi = qt * 32 * NW + qrow;
      if (qi < Lq) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(so + (pl * 32 * NW + qrow) * 128 + ((piece ^ ((qrow >> 1) & 7)) << 4));
        *reinterpret_cast<u32x4*>(p.out2 + (long)pl * p.out2_plane + (rowbase + qi) * p.ldo + h * 64 + piece * 8) = v;
      }
    }
  } else {
    const int qi = q0 + r32;
    if (active && qi < Lq) store_o_f32(p.out + (rowbase + qi) * p.ldo + h * 64 + 4 * half, o0, o1, inv);
  }
}

template <int NW, int NST = PL_NSTAGE>
void launch_pl(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(cdiv(a.L, 32 * NW) * a.H * a.B);
  if (a.np == 1) hipLaunchKernelGGL((attn64_pl_kernel<NW, NST, 1>), grid, dim3(64 * NW), 0, st, a);
  else hipLaunchKernelGGL((attn64_pl_kernel<NW, NST>), grid, dim3(64 * NW), 0, st, a);
}

}  // namespace

// q: fp32 rows (a.qkv, a.ld); K / V: fp16 planes of k * k_scale / v * v_scale at a.kv2 ([2][rows][kv_ld], K at column 0, V at
// column 512, head h at + 64 h).  Same contract as attention64() otherwise.
int attention64_planes(const AttnArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.L <= 0) return JV_OK;
  JV_TRY(attn_planes_check(a, "attention64_planes", true));
  int nw = a.L <= 64 ? 2 : (round_up(a.L, 256) == round_up(a.L, 128) ? 8 : 4);
  if (const char* f = dyn_env("JV_ATTN_NW")) nw = atoi(f);
  if (nw != 2 && nw != 4) nw = 8;
  static const char* const names[9] = {"", "", "attn64_pl<2 waves>", "", "attn64_pl<4 waves>", "", "", "", "attn64_pl<8 waves>"};
  static const char* const names1[9] = {"", "", "attn64_pl<2 waves,np1>", "", "attn64_pl<4 waves,np1>", "", "", "", "attn64_pl<8 waves,np1>"};
  return attn_bracket(a, st, (a.np == 1 ? names1 : names)[nw], [&] {
    if (nw == 2) launch_pl<2>(a, st);
    // two stages (32 KB, <= 128 VGPRs): four workgroups per CU instead of three -- the fourth hides more of the others'
    // barriers and softmax chains than the third stage hid of the DMA latency (175.1 -> 171.7 ms per pass, same box)
    else if (nw == 4 && dyn_env("JV_ATTN_NST3")) launch_pl<4, 3>(a, st);
    else if (nw == 4) launch_pl<4, 2>(a, st);
    else launch_pl<8>(a, st);
  });
}

}  // namespace jv
