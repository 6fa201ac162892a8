// fp16x3 self-attention of the estimator, third form: ONE workgroup per (utterance, head, 64 QT queries), each of its four
// waves owning 16 QT queries (QT = 5: 80 queries per wave, 320 per workgroup -- a whole 300-frame head) against every key.
// jyutvoice/flow/transformer.py:380-389 -> diffusers AttnProcessor2_0 as restated in oracle/flow.py:46-58.
//
// Why a third kernel.  attn64_pl_kernel (attention_pl.hip) gives a wave ONE 32-query tile: per 32-key tile it reads the whole
// K / V tile from LDS for 24 MFMAs, passes a barrier, issues its share of the next tile's DMA, and runs a softmax whose
// instructions cannot overlap the wave's own MFMAs -- measured (profiles/r02_pmc_attention_pl.md) 10.7 vector instructions
// per MFMA, the matrix pipe 27 % busy; and a 300-frame head is 10 such tiles = 2.5 four-wave workgroups, so a launch is 1.5
// rounds of workgroups with the last one per head mostly idle.  Here:
//   * a wave's K fragment (16 keys x 32 d) and V^T fragment (16 d x 32 keys) are read ONCE per key tile and used for all QT
//     query tiles: LDS reads, barriers, DMA issues and loop overhead per MFMA drop QT-fold;
//   * v_mfma_f32_16x16x32_f16: 16-query granularity is what lets 80-query waves exist (300 = 3.75 x 80); S^T[key][query]
//     again, so softmax statistics are per lane (query = lane & 15) and P is directly the B operand of O^T = V^T P^T:
//     lane group kq = lane >> 4 holds keys 4 kq + e of the two 16-key blocks, which is the key order the transposing
//     ds_read_b64_tr_b16 delivers V^T in;
//   * the row sum of P stays a per-lane partial (this lane's keys) until the end: one cross-lane reduction per query and
//     launch instead of one per key tile; only the running maximum crosses lanes per tile (two row / half exchanges);
//   * 512 workgroups at 32 x 300 frames = two per CU, one round.
// Arithmetic: attention_common.h's pieces, as in attention_pl.hip (scales, base-2 softmax on raw v_exp_f32, P kept as p * 2^10, products hh' + hl' + lh'
// smallest first); the contraction over d runs in two 32-deep MFMAs instead of four 16-deep ones and the row sums are
// grouped per lane, so results agree with that kernel to rounding, not bit for bit.
#include <math.h>
#include <stdlib.h>

#include "attention_common.h"
#include "row_mainloop.h"      // h3_mma: the fp16x3 step on v_mfma_f32_16x16x32_f16

namespace jv {

namespace {

constexpr int AR_NW = 4;

template <int QT, int NST>
__global__ __launch_bounds__(64 * AR_NW, 2) void attn64_r_kernel(const AttnArgs p) {
  // the K / V ring; after the key loop each wave's [2 planes][16 queries][128 B] output patch (4 KB per wave)
  __shared__ __attribute__((aligned(256))) unsigned char lds[NST * KV_STAGE];
  static_assert(NST * KV_STAGE >= AR_NW * 2 * 16 * 128, "the output patches fit the ring");
  constexpr int PPW = 16 / AR_NW;      // DMA pieces per wave and key tile
  constexpr int QW = 16 * QT;          // queries per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int nqt = (p.L + AR_NW * QW - 1) / (AR_NW * QW);      // workgroups per head
  const int qt = blockIdx.x % nqt;
  const int h = (blockIdx.x / nqt) % p.H;
  const int b = blockIdx.x / (nqt * p.H);
  const int q0 = qt * AR_NW * QW + wave * QW;
  const int len = p.lens ? min(p.lens[b], p.L) : p.L;
  const long rowbase = (long)p.G + (long)b * p.S;
  const bool active = q0 < p.L;

  // ---- this wave's DMA pieces of a key tile (attention_common.h: kv_piece)
  const unsigned short* src[PPW];
  int dst[PPW], krel[PPW];
  const int kstride = p.kv_ld;
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const KvPiece pc = kv_piece(wave + AR_NW * i, lane);
    const int slot = kv_slot<VT_8x32>(pc.opv, pc.krel, lane);
    krel[i] = pc.krel;
    src[i] = p.kv2 + (long)pc.pl * p.kv2_plane + rowbase * kstride + pc.opv * 512 + h * 64 + 8 * slot;
    dst[i] = pc.dst;
  }
  auto issue = [&](int k0, int stage) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) kv_issue_piece(src[i], dst[i], krel[i], kstride, k0, len, lds + stage * KV_STAGE);
  };
  const int nkt = (len + 31) >> 5;
  if (nkt > 0) issue(0, 0);
  if (NST > 2 && nkt > 1) issue(32, 1);

  // ---- Q planes: B operand of S^T = K Q^T.  Lane (query r16, kq) holds d = 32 ds + 8 kq + j, pre-scaled by log2(e) / 8 * q_scale
  u32x4 qf[QT][2][2];
  const float qsc = q_prescale(p.q_scale);
  const float sinv = 1.0f / (p.q_scale * p.k_scale);      // powers of two: exact
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = q0 + 16 * t + r16;
    const float* qs = p.qkv + (rowbase + qi) * p.ld + h * 64 + 8 * kq;
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
      if (qi < p.L) {
        t0 = *reinterpret_cast<const f32x4*>(qs + 32 * ds);
        t1 = *reinterpret_cast<const f32x4*>(qs + 32 * ds + 4);
      }
      q_split8(t0, t1, qsc, qf[t][ds][0], qf[t][ds][1]);
    }
  }

  f32x4 o[QT][4];      // O^T[d = 16 db + 4 kq + e][query r16]
  float m_run[QT], l_run[QT];      // l_run: THIS LANE's keys only (reduced over the four lanes of a query at the end)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[t][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // per-lane read offsets inside a stage
  const int k_row = r16 * 128;                                   // K: + kb * 2048 + pl * KV_PLANE + slot
  const int vq = r16 >> 2, vp = lane & 3;                        // V^T: key within its 4-block, 8-byte piece (4 d)
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * 32;
    if (NST > 2 && kt + 1 < nkt) wait_vmcnt<PPW>(); else wait_vmcnt<0>();
    bare_barrier();
    if (NST > 2) { if (kt + 2 < nkt) issue(k0 + 64, (kt + 2) % NST); }
    else if (kt + 1 < nkt) issue(k0 + 32, (kt + 1) % NST);
    if (!active) continue;
    const unsigned char* const sK = lds + (kt % NST) * KV_STAGE;
    const unsigned char* const sV = sK + 2 * KV_PLANE;

    // ---- S^T[key][query] = sum_d K[key][d] Q[query][d]: each K fragment read once, used by all QT query tiles
    f32x4 s[QT][2];
#pragma unroll
    for (int t = 0; t < QT; ++t) { s[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; s[t][1] = s[t][0]; }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ds = 0; ds < 2; ++ds) {
        u32x4 a[2];
        const int key = 16 * kb + r16;
        const int ko = ((4 * ds + kq) ^ kv_k_swz(key)) << 4;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a[pl] = *reinterpret_cast<const u32x4*>(sK + pl * KV_PLANE + kb * 2048 + k_row + ko);
#pragma unroll
        for (int t = 0; t < QT; ++t) s[t][kb] = h3_mma(s[t][kb], a[0], a[1], qf[t][ds][0], qf[t][ds][1]);
      }

    // ---- softmax (base 2), per query tile; P leaves as the B operand of the PV product
    const bool edge = k0 + 32 > len;      // (wave-uniform) only the last tile can straddle the key mask
    u32x4 pb[QT][2];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (edge) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[t][kb][e] = (k0 + 16 * kb + 4 * kq + e) < len ? s[t][kb][e] : -INFINITY;
      }
      float mt = fmaxf(fmaxf(fmaxf(s[t][0][0], s[t][0][1]), fmaxf(s[t][0][2], s[t][0][3])),
                       fmaxf(fmaxf(s[t][1][0], s[t][1][1]), fmaxf(s[t][1][2], s[t][1][3])));
      mt = q_max(mt) * sinv;
      const float m_new = fmaxf(m_run[t], mt);
      const float alpha = __builtin_amdgcn_exp2f(m_run[t] - m_new);
      float lt = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[t][kb][e] = __builtin_amdgcn_exp2f(fmaf(s[t][kb][e], sinv, 10.f - m_new));      // p * 2^10 (cancels in 1 / l)
          lt += s[t][kb][e];
        }
      l_run[t] = l_run[t] * alpha + lt;
      m_run[t] = m_new;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int db = 0; db < 4; ++db) o[t][db] = o[t][db] * alpha;
      }
      // k-slot j of lane group kq: j < 4 -> key 4 kq + j of block 0, j >= 4 -> key 4 kq + j - 4 of block 1
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const Split2 sp = split2h_pair(s[t][kb][e], s[t][kb][e + 1]);
          pb[t][0][2 * kb + (e >> 1)] = sp.h;
          pb[t][1][2 * kb + (e >> 1)] = sp.l;
        }
    }

    // ---- O^T[d][query] += sum_key V[key][d] P[query][key]: each V^T fragment read once (transposing read), used by all tiles
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      u32x4 a[2];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
          const int key = 16 * rd + 4 * kq + vq;
          const int byte = (16 * db + 4 * vp) * 2;
          const u32x2 u = vt_read4(sV + pl * KV_PLANE + vt_off(key, byte, kv_v_swz<VT_8x32>(key)));
          a[pl][2 * rd] = u[0];
          a[pl][2 * rd + 1] = u[1];
        }
#pragma unroll
      for (int t = 0; t < QT; ++t) o[t][db] = h3_mma(o[t][db], a[0], a[1], pb[t][0], pb[t][1]);
    }
  }

  // ---- result: O / l as the output projection's operand (fp16 planes), each wave through its own 4 KB patch of the idle
  // ring so that every store instruction writes whole 128-byte rows
  lds_barrier();      // every wave is done with the ring
  if (!active) return;
  unsigned char* const so = lds + wave * (2 * 16 * 128);      // [2 planes][16 queries][128 B]
  const float vsc = p.v_scale;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const float l = q_sum(l_run[t]);
    const float inv = l > 0.f ? (1.0f / vsc) / l : 0.f;
    const int qbase = q0 + 16 * t;
    if (qbase >= p.L) break;      // (wave-uniform)
    if (p.out2) {
      const float sc = inv * p.out2_scale;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const Split2 a0 = split2h_pair(o[t][db][0] * sc, o[t][db][1] * sc);
        const Split2 a1 = split2h_pair(o[t][db][2] * sc, o[t][db][3] * sc);
        unsigned char* dp = so + r16 * 128 + (16 * db + 4 * kq) * 2;      // 4 consecutive d: 8 bytes
        *reinterpret_cast<u32x2*>(dp) = u32x2{a0.h, a1.h};
        *reinterpret_cast<u32x2*>(dp + 16 * 128) = u32x2{a0.l, a1.l};
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (a wave's LDS accesses execute in order; the reads below see these writes)
      // 8 lanes per row of 128 B, 8 rows per instruction: 2 planes x 16 rows = 4 instructions
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int pl = it >> 1, qrow = (it & 1) * 8 + (lane >> 3), piece = lane & 7;
        const int qi = qbase + qrow;
        const u32x4 v = *reinterpret_cast<const u32x4*>(so + (pl * 16 + qrow) * 128 + piece * 16);
        if (qi < p.L) *reinterpret_cast<u32x4*>(p.out2 + (long)pl * p.out2_plane + (rowbase + qi) * p.ldo + h * 64 + piece * 8) = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the patch is rewritten by the next tile
    } else {
      const int qi = qbase + r16;
      if (qi < p.L) {
        float* dp = p.out + (rowbase + qi) * p.ldo + h * 64 + 4 * kq;
#pragma unroll
        for (int db = 0; db < 4; ++db) *reinterpret_cast<f32x4*>(dp + 16 * db) = o[t][db] * inv;
      }
    }
  }
}

template <int QT, int NST>
void launch_r(const AttnArgs& a, hipStream_t st) {
  const int nqt = cdiv(a.L, AR_NW * 16 * QT);
  hipLaunchKernelGGL((attn64_r_kernel<QT, NST>), dim3(nqt * a.H * a.B), dim3(64 * AR_NW), 0, st, a);
}

}  // namespace

// same contract as attention64_planes() (attention_pl.hip); no chunk-causal mask (streaming stays on attention64_planes)
int attention64_rows(const AttnArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.L <= 0) return JV_OK;
  JV_TRY(attn_planes_check(a, "attention64_rows", false));
  int qt = attention64_tiles(a.L);
  if (const char* f = dyn_env("JV_ATTN_QT")) qt = atoi(f);
  const bool st3 = dyn_env("JV_ATTN_NST2") == nullptr;
  static const char* const names[6] = {"", "", "attn64_r<128 q>", "attn64_r<192 q>", "attn64_r<256 q>", "attn64_r<320 q>"};
  return dispatch_rt(qt, "attention64_rows: bad tile count", [&](auto qc) {
    return attn_bracket(a, st, names[qc], [&] {
      if (st3) launch_r<decltype(qc)::value, 3>(a, st);
      else launch_r<decltype(qc)::value, 2>(a, st);
    });
  });
}

}  // namespace jv
