// Column-slab copies between [rows, C, width] fp32 buffers (jv_slab_copy): the state moves of a batch of streaming sessions --
// append a mel piece to a slot's record, gather the ragged windows of a step, crop what a window keeps -- as ONE launch for all
// sessions of the step, whatever their number.  Bandwidth-trivial; what matters is that every column offset works.
//
// A descriptor is five ints (src_row, src_col, dst_row, dst_col, n): dst[dst_row, :, dst_col + j] = src[src_row, :, src_col + j]
// for j < n and, with zero_fill, 0 for n <= j < span (cut at the destination's width).  A descriptor that does not fit its buffers
// (a row or column range outside them, n < 0, n > span) moves nothing at all: the descriptors live on the device, so the kernel
// is the only place that can check them.  n < 0 is how a caller marks a row that has nothing to do.
//
// 16-byte accesses where the addresses allow: a thread owns four consecutive destination floats starting on a 16-byte boundary of
// the DESTINATION (the first thread of a slab takes the 0 .. 3 floats ahead of the first boundary), stores them as one f32x4 when
// all four are inside the slab, and loads them as one f32x4 when the source address is aligned too -- else as four dwords.
#include "../../include/jyutvoice_hip.h"
#include "jv_model.h"

namespace jv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void slab_copy_kernel(const float* __restrict__ src, int src_rows, int src_width,
                                                        float* __restrict__ dst, int dst_rows, int dst_width, int C,
                                                        const int* __restrict__ desc, int span, int zero_fill, int vec_ok) {
  const int* d = desc + 5 * (long)blockIdx.z;
  const int sr = d[0], sc = d[1], dr = d[2], dc = d[3], n = d[4];
  if (n < 0 || n > span || sr < 0 || sr >= src_rows || dr < 0 || dr >= dst_rows || sc < 0 || dc < 0 ||
      (long)sc + n > src_width || (long)dc + n > dst_width)
    return;
  const int c = blockIdx.y;
  const int limit = zero_fill ? min(span, dst_width - dc) : n;      // destination columns this descriptor writes
  const long soff = ((long)sr * C + c) * src_width + sc, doff = ((long)dr * C + c) * dst_width + dc;
  const float* s = src + soff;
  float* o = dst + doff;
  const int head = (int)((4 - (doff & 3)) & 3);      // floats ahead of the destination's first 16-byte boundary
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long e0 = i == 0 ? 0 : head + 4 * (i - 1);
  const int cnt = i == 0 ? head : 4;
  if (e0 >= limit) return;
  if (vec_ok && cnt == 4 && e0 + 4 <= limit) {
    f32x4 v;
    if (e0 + 4 <= n && ((soff + e0) & 3) == 0) {
      v = *reinterpret_cast<const f32x4*>(s + e0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = e0 + j < n ? s[e0 + j] : 0.f;
    }
    *reinterpret_cast<f32x4*>(o + e0) = v;
    return;
  }
  for (int j = 0; j < cnt && e0 + j < limit; ++j) o[e0 + j] = e0 + j < n ? s[e0 + j] : 0.f;
}

}  // namespace jv

extern "C" int jv_slab_copy(jv_context* ctx, const float* src, int src_rows, int src_width, float* dst, int dst_rows, int dst_width,
                            int C, const int32_t* desc, int B, int span, int zero_fill, void* stream) {
  if (!ctx || !src || !dst || !desc) return jv::fail(JV_ERR_ARG, "jv_slab_copy: null argument");
  if (src_rows < 1 || dst_rows < 1 || src_width < 0 || dst_width < 0 || C < 1 || C > 65535 || B < 0 || B > 65535 || span < 0)
    return jv::fail(JV_ERR_ARG, "jv_slab_copy: rows and C must be positive (C, B <= 65535), widths, B and span non-negative");
  if ((const void*)src == (const void*)dst) return jv::fail(JV_ERR_ARG, "jv_slab_copy: source and destination must be different buffers");
  JV_HIP(hipSetDevice(ctx->c.device));
  if (B == 0 || span == 0) return JV_OK;
  // base pointers off a 16-byte boundary (a view into a tensor): every access is a dword
  const int vec_ok = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const unsigned gx = (unsigned)jv::cdivl(1 + jv::cdivl(span, 4) + 1, 256);      // the head thread + the quads (+ one for a cut quad)
  hipLaunchKernelGGL(jv::slab_copy_kernel, dim3(gx, (unsigned)C, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                     src_rows, src_width, dst, dst_rows, dst_width, C, desc, span, zero_fill ? 1 : 0, vec_ok);
  JV_HIP(hipGetLastError());
  return JV_OK;
}
