// The shared pieces of the four hand-scheduled attention kernels -- attn64_x6_kernel (attention.hip), attn64_pl_kernel
// (attention_pl.hip), attn64_s_kernel (attention_s.hip), attn64_r_kernel (attention_r.hip) -- in ONE place: the K / V ring's
// tile geometry, slot keys and LDS-DMA piece table, the lane exchanges, the fp16x3 step, the Q split, the transposed V
// fragment read, the geometries, the fp32 epilogue and the host side's checks and profiler bracket.  The four files are four
// SCHEDULES over these pieces.  As in row_tail.h and row_mainloop.h the pieces take and return values or references;
// addresses that are a kernel's own, the derivation of its wait counts and the PLACE AND ORDER of every load, wait and
// barrier stay in the kernels.
//
// The bit contract between attn64_pl and attn64_s (tests: test_attention_single_equals_planes_bit_for_bit -- an utterance's
// mel must not depend on which of the two its batch size selects) rests on what is written here once and called by both:
//   * the Q operand: q_split8 with the same scale log2(e) / 8 * q_scale (q_prescale), the same split;
//   * every product: h3_mma32's term order (lo hi, hi lo, hi hi).  attn64_s issues the three MFMAs as asm on named AGPRs and
//     therefore writes the order out (qk_mfma / pv_mfma, term 0 .. 2): those are the lines to keep equal to h3_mma32;
//   * the softmax: attn_lazy_max (jv_device.h), half_max / half_sum over a query's two lanes, P kept as p * 2^10;
//   * the K / V bytes: one piece decode (kv_piece, kv_slot, kv_issue_piece), one K slot key, one V slot key per read pattern.
// Kept written out on purpose (profiles/attention_common_isa.md has what each one cost as a helper, shape by shape):
//   * the piece table as ONE struct, the V^T byte offset (vt_off: attn64_r calls it, attn64_pl and attn64_s spell it out), the
//     two transposing reads as one call, AttnGeo in attn64_pl, store_o_f32 in attn64_x6: each changed a default-route
//     kernel's instruction mix, main-loop instruction count or registers.  The compiler simplifies a helper on its own
//     before it inlines it, without the ranges (lane < 64, wave < NW) the kernel's context gives the same expression;
//   * attn64_s: its fragment reads and MFMAs (asm on AGPRs the compiler does not know about), the maximum on v_max3
//     (as_max3: no canonicalising v_max), its Q fetch pipeline and LDS patch, its rotated loop;
//   * attn64_r: its uniform-only geometry and its per-lane row sums; attention.hip: the bf16x6 arm and its own V^T staging.
#pragma once
#include "jv_common.h"
#include "jv_device.h"
#include "jv_launch.h"

namespace jv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int KV_PLANE = 32 * 128;                 // one plane of a 32-key tile: 128 bytes (64 d) per key
constexpr int KV_STAGE = 4 * KV_PLANE;             // K h, K l, V h, V l

// ---- 16-byte slot keys of a key row (128 B = 8 slots), brute-forced against the LDS lane groups of MI355X_MICROARCH.md ----
// K is read by rows (ds_read_b128, lane = key): a lane group holds every key parity twice per value of (key >> 1) & 7
__device__ __forceinline__ int kv_k_swz(int key) { return (key >> 1) & 7; }
// V is read transposed (ds_read_b64_tr_b16), and the key depends on what a 32-lane half of that read covers:
enum VtRead {
  // 4 consecutive keys x 64 contiguous bytes (32x32x16 MFMAs: attn64_pl, attn64_s): swapping the row's 64-byte halves on
  // keys with bit 1 set puts the four rows on the four 64-byte quarters of the 256-byte bank row (conflict-free)
  VT_4x64,
  // 8 keys x 32 contiguous bytes (16x16x32 MFMAs: attn64_r): a different key ON PURPOSE -- the eight rows go to the eight
  // 32-byte pieces of the bank row
  VT_8x32
};
template <VtRead R>
__device__ __forceinline__ int kv_v_swz(int key) { return R == VT_4x64 ? ((key >> 1) & 1) << 2 : ((key >> 1) & 3) << 1; }

// ---- lane exchanges.  combine a value with its partner lane's (lane ^ 32: the two lanes that hold one query's keys) in one
// VALU op: v_permlane32_swap_b32 (gfx950) returns {own half | partner's low half, partner's high half | own}; ds_bpermute,
// what __shfl_xor compiles to, is an LDS round trip
__device__ __forceinline__ float half_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// max / sum over the four lanes that share a query (lane, lane ^ 16, lane ^ 32, lane ^ 48), in every one of them
__device__ __forceinline__ float q_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return half_max(fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])));
}
__device__ __forceinline__ float q_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return half_sum(__uint_as_float(a[0]) + __uint_as_float(a[1]));
}

// ---- fp16x3 on v_mfma_f32_32x32x16_f16: c + (a_hi + a_lo)(b_hi + b_lo) without the lo lo term, smallest terms first (the
// 16x16x32 twin is h3_mma of row_mainloop.h); NP = 1: the hi hi product alone (the estimator's FP16 mode) ----
template <int NP = 3>
__device__ __forceinline__ f32x16 h3_mma32(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x16 c) {
  auto mm = [&](const u32x4& x, const u32x4& y) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), c, 0, 0, 0);
  };
  static_assert(NP == 3 || NP == 1, "three products or the hi hi product alone");
  if constexpr (NP == 3) {
    mm(a[1], b[0]);
    mm(a[0], b[1]);
  }
  mm(a[0], b[0]);
  return c;
}

// ---- the Q operand: pre-scaled by log2(e) / 8 * q_scale (scores come out in base-2 units: one v_exp_f32 per element), and the
// eight values a lane holds of one k-step (two f32x4 of its row) as one dword quadruple per plane ----
__device__ __forceinline__ float q_prescale(const float q_scale) { return 0.125f * 1.44269504088896340736f * q_scale; }
__device__ __forceinline__ void q_split8(const f32x4& t0, const f32x4& t1, const float scale, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x0 = (e < 2 ? t0[2 * e] : t1[2 * e - 4]) * scale, x1 = (e < 2 ? t0[2 * e + 1] : t1[2 * e - 3]) * scale;
    const Split2 t = split2h_pair(x0, x1);
    hi[e] = t.h;
    lo[e] = t.l;
  }
}

// ---- a wave's LDS-DMA pieces of a 32-key tile (16 one-KiB pieces: global_load_lds_dwordx4, a wave per piece) ----
// piece pc = wave + NW i (NW waves, 16 / NW pieces per wave: what a kernel's counted vmcnt waits are made of) -> operand
// pc >> 3 (K, V), plane (pc >> 2) & 1, 8-key group pc & 3; lane L lands on key 8 g + (L >> 3), slot L & 7 and therefore
// FETCHES the slot the read side's key maps there.  A kernel keeps src[], dst[], krel[] of its pieces and the line that
// forms a piece's global address; it decides when to issue, and the stage's base address is its own.
// (As ONE struct -- the three arrays, init(), issue() -- or as one decode function that also returns the slot, the table
// changed attn64_pl's and attn64_s's main-loop instruction counts and attn64_pl<8, 3>'s registers; in these three pieces the
// two kernels keep the parent's code: profiles/attention_common_isa.md.)
struct KvPiece { int opv, pl, krel, dst; };      // operand, plane, key inside the tile, byte offset inside a stage
__device__ __forceinline__ KvPiece kv_piece(const int pc, const int lane) {
  const int opv = pc >> 3, pl = (pc >> 2) & 1, g = pc & 3;
  return {opv, pl, 8 * g + (lane >> 3), (2 * opv + pl) * KV_PLANE + g * 1024};
}
template <VtRead VR>
__device__ __forceinline__ int kv_slot(const int opv, const int key, const int lane) { return (lane & 7) ^ (opv ? kv_v_swz<VR>(key) : kv_k_swz(key)); }
// rows past the last valid key are clamped to it: their scores are masked to -inf by the kernel, P is exactly 0 there
__device__ __forceinline__ void kv_issue_piece(const unsigned short* const src, const int dst, const int krel, const int kstride, const int k0,
                                               const int len, unsigned char* const stage_base) {
  const int key = min(k0 + krel, len - 1);
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long)key * kstride),
                                   (__attribute__((address_space(3))) void*)(stage_base + dst), 16, 0, 0);
}

// ---- the transposed V fragment.  V stays row-major [key][128 B] in LDS (what the DMA can deliver); the PV product's A
// operand, 8 keys of one d, is two ds_read_b64_tr_b16 of 4 keys each.  Byte offset of `byte` of key `key` under slot key swz
// (attn64_pl and attn64_s keep this expression written out: as a call it changed their instruction mix, and attn64_s's
// main-loop counts at four and five query tiles):
__device__ __forceinline__ int vt_off(const int key, const int byte, const int swz) {
  return key * 128 + ((((byte >> 4) ^ swz) << 4) | (byte & 15));
}
// one of the two reads: 4 keys x 4 d -> the two dwords of the fragment's half.  (As ONE call that takes both offsets and returns
// the u32x4, attn64_pl<4, 2>'s main loop came out one instruction shorter and two registers smaller -- not the parent's code.)
__device__ __forceinline__ u32x2 vt_read4(const unsigned char* const at) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)const_cast<unsigned char*>(at)));
}

// ---- geometry ----
// flat block id -> the id whose (b, h, q-tile) triple it takes, so that each XCD gets a contiguous run of triples with the
// q-tile fastest: the q-tiles of one (b, h) then share that head's K / V in one L2 (round 1: FETCH_SIZE was 2.3x the
// algorithmic bytes)
__device__ __forceinline__ int xcd_remap(const int bid, const int nwg) {
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
}
// utterance b's valid keys, first row and query count.  Uniform geometry: row G + b S, L queries.  Compact geometry
// (AttnArgs::uoff): the utterance owns len rows; what lies behind them is the next utterance.  (attn64_s constructs it;
// attn64_pl keeps the same three lines written out: there every helper shape changed the prologue's instruction mix.)
struct AttnGeo {
  int len;
  long rowbase;
  int Lq;
  __device__ __forceinline__ AttnGeo(const AttnArgs& p, const int b)
      : len(p.lens ? min(p.lens[b], p.L) : p.L), rowbase(p.uoff ? (long)p.uoff[b] : (long)p.G + (long)b * p.S), Lq(p.uoff ? len : p.L) {}
};

// ---- fp32 output of the 32x32 O^T accumulator pair (d 0..31 / 32..63 of a lane's query); dst: the query's row + 4 half ----
// (attn64_pl and the fp32 attn64_kernel; attn64_x6_kernel keeps the loop written out: see there)
__device__ __forceinline__ void store_o_f32(float* const dst, const f32x16& o0, const f32x16& o1, const float inv) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 a = {o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv};
    const f32x4 c = {o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv};
    *reinterpret_cast<f32x4*>(dst + 8 * g) = a;
    *reinterpret_cast<f32x4*>(dst + 32 + 8 * g) = c;
  }
}

// ---- host side of the three plane-fed forms (attention64_planes, attention64_rows, attention64_single) ----
inline int attn_planes_check(const AttnArgs& a, const char* name, const bool allow_chunk) {
  if (!a.kv2 || (a.kv_ld & 7) || !(a.q_scale > 0.f && a.k_scale > 0.f && a.v_scale > 0.f) || (a.ld & 3) || (a.ldo & 7) ||
      (!allow_chunk && a.chunk > 0))
    return fail(JV_ERR_ARG, std::string(name) + ": needs K/V planes, the three scales, aligned strides" + (allow_chunk ? "" : ", no chunk mask"));
  return JV_OK;
}
// launch() between the profiler's events, under `name` with the algorithmic (full-length) figure of SURVEY.md 8(d):
// QK^T + PV = 4 L L 64 per head; q, k, v, o once
template <class Launch>
int attn_bracket(const AttnArgs& a, hipStream_t st, const char* name, Launch&& launch) {
  const bool prof = prof_on();
  if (prof) prof_begin(st);
  launch();
  if (prof) {
    const double bh = (double)a.B * a.H;
    prof_end(st, name, 4.0 * bh * a.L * a.L * 64.0, 4.0 * bh * a.L * 64.0 * 4.0);
  }
  JV_HIP(hipGetLastError());
  return JV_OK;
}
// queries per workgroup = 64 QT (attn64_r, attn64_s): the QT in {2 .. 5} that covers L with the fewest padded queries
// (workgroups x 64 QT), the taller tile on a tie (each K / V fragment is then used for more queries).  300 frames -> 5,
// 512 -> 4, 128 -> 2
inline int attention64_tiles(const int L) {
  int best = 5;
  long best_q = 1L << 40;
  for (int qt = 5; qt >= 2; --qt) {
    const long padded = (long)cdiv(L, 64 * qt) * 64 * qt;
    if (padded < best_q) { best = qt; best_q = padded; }
  }
  return best;
}

}  // namespace jv
