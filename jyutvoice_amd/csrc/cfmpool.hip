// In-flight batching of the CFM solve (flow.hip cfm_pool_*; jv_cfm_pool_admit / _step / _fetch): the moves between the caller's
// request pools and the solver's row buffers.  A request's state is its x, mu and cond rows ([slots, Tcap, 80], frame-major), its
// projected speaker vector and six running maxima; a step gathers the listed slots into the workspace in either row geometry, and
// after the estimator applies the Euler + CFG update with the request's OWN dt -- or a stage of the request's own midpoint / Heun
// step (pool_stage_scatter) -- straight into the pool.  Bandwidth-trivial, 16 B
// per lane.  What the host decides per call arrives as kernel arguments (jv_ops.h: Pool*Chunk), one launch per POOL_CHUNK requests
// where the arguments are read by the kernel itself; every index was validated on the host before the first launch.
#include "jv_common.h"
#include "jv_ops.h"

namespace jv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- admit: the prompted pack of rowops.hip (pack_prompted_kernel) + the scaled noise prefix, into pool slots --------------
// Frame t < p copies prompt_h[b, t, :] / prompt_feat[b, t, :]; frame p <= t < len takes mu_y[b, :, t - p] through an LDS tile (read
// along t, written along c) and zeros in cond; x[t, c] = noise[c, t] * temp through a second tile (the product cf_to_rows forms).
__global__ __launch_bounds__(256) void pool_admit_kernel(const PoolAdmitChunk ch, const float* __restrict__ mu_y, int Ty,
                                                         const float* __restrict__ prompt_h, int Ph,
                                                         const float* __restrict__ prompt_feat, int Pf,
                                                         const float* __restrict__ spks, const float* __restrict__ noise,
                                                         long noise_pitch, float* __restrict__ pool_x, float* __restrict__ pool_mu,
                                                         float* __restrict__ pool_cond, float* __restrict__ pool_spks,
                                                         float* __restrict__ pool_amax, int Tcap) {
  __shared__ float tm[32][81], tn[32][81];
  const int i = blockIdx.y, b = ch.b0 + i, t0 = blockIdx.x * 32;
  const int slot = ch.r[i].slot, p = ch.r[i].p, len = ch.r[i].len;
  const float temp = ch.r[i].temp;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 20)
      *reinterpret_cast<f32x4*>(pool_spks + (long)slot * 80 + 4 * threadIdx.x) = *reinterpret_cast<const f32x4*>(spks + (long)b * 80 + 4 * threadIdx.x);
    else if (threadIdx.x >= 64 && threadIdx.x < 70)
      pool_amax[(long)slot * 6 + (threadIdx.x - 64)] = 0.f;      // the slot's previous occupant leaves nothing behind
  }
  if (t0 >= len) return;      // (uniform over the block)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  {
    const int t = t0 + tx;
    const bool text = t >= p && t < len;
    for (int c = ty; c < 80; c += 8) {
      tm[tx][c] = text ? mu_y[((long)b * 80 + c) * Ty + (t - p)] : 0.f;
      tn[tx][c] = t < len ? noise[(long)c * noise_pitch + t] * temp : 0.f;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 32 * 20; idx += 256) {
    const int r = idx / 20, q = idx - r * 20, t = t0 + r;
    if (t >= len) continue;
    f32x4 m = {tm[r][4 * q], tm[r][4 * q + 1], tm[r][4 * q + 2], tm[r][4 * q + 3]}, cd = {0.f, 0.f, 0.f, 0.f};
    if (t < p) {
      m = *reinterpret_cast<const f32x4*>(prompt_h + ((long)b * Ph + t) * 80 + 4 * q);
      cd = *reinterpret_cast<const f32x4*>(prompt_feat + ((long)b * Pf + t) * 80 + 4 * q);
    }
    const long o = ((long)slot * Tcap + t) * 80 + 4 * q;
    *reinterpret_cast<f32x4*>(pool_mu + o) = m;
    *reinterpret_cast<f32x4*>(pool_cond + o) = cd;
    *reinterpret_cast<f32x4*>(pool_x + o) = f32x4{tn[r][4 * q], tn[r][4 * q + 1], tn[r][4 * q + 2], tn[r][4 * q + 3]};
  }
}

int pool_admit(const PoolAdmitChunk& ch, int tmax, const float* mu_y, int Ty, const float* prompt_h, int Ph, const float* prompt_feat,
               int Pf, const float* spks, const float* noise, long noise_pitch, float* pool_x, float* pool_mu, float* pool_cond,
               float* pool_spks, float* pool_amax, int Tcap, hipStream_t st) {
  if (ch.n <= 0 || tmax <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_admit_kernel, dim3(cdiv(tmax, 32), ch.n), dim3(256), 0, st, ch, mu_y, Ty, prompt_h, Ph, prompt_feat, Pf,
                     spks, noise, noise_pitch, pool_x, pool_mu, pool_cond, pool_spks, pool_amax, Tcap);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// ---- a step's tables: the estimator, the row tables and the kernels below read them from the device ----------------------------
__global__ void pool_publish_kernel(const PoolStepChunk ch, int B, PoolStepReq* __restrict__ req, int* __restrict__ lens2,
                                    float* __restrict__ t_dev, int* __restrict__ uoff, int rows_end) {
  const int i = threadIdx.x;
  if (i >= ch.n) return;
  const int b = ch.b0 + i;
  const PoolStepReq r = ch.r[i];
  req[b] = r;
  lens2[b] = lens2[B + b] = r.len;
  t_dev[b] = t_dev[B + b] = r.t;
  if (uoff) {
    uoff[b] = r.row;
    uoff[B + b] = r.rowu;
    if (b == B - 1) uoff[2 * B] = rows_end;
  }
}

int pool_publish(const PoolStepChunk& ch, int B, PoolStepReq* req, int* lens2, float* t_dev, int* uoff, int rows_end, hipStream_t st) {
  if (ch.n <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_publish_kernel, dim3(1), dim3(POOL_CHUNK), 0, st, ch, B, req, lens2, t_dev, uoff, rows_end);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// ---- gather: pool slots -> the conditional rows of the step (the twins' x / mu / cond rows are never read: assemble_xin takes a
// twin's x from its request's row and nothing else) ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pool_gather_kernel(const PoolStepReq* __restrict__ req, int B, int tfill,
                                                          const float* __restrict__ pool_x, const float* __restrict__ pool_mu,
                                                          const float* __restrict__ pool_cond, const float* __restrict__ pool_spks,
                                                          const float* __restrict__ pool_amax, int Tcap, float* __restrict__ x,
                                                          float* __restrict__ mu, float* __restrict__ cond, float* __restrict__ spks,
                                                          float* __restrict__ amax, int amax_stride) {
  const int b = blockIdx.y;
  const int slot = req[b].slot, len = req[b].len;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 20)
      *reinterpret_cast<f32x4*>(spks + (long)b * 80 + 4 * threadIdx.x) = *reinterpret_cast<const f32x4*>(pool_spks + (long)slot * 80 + 4 * threadIdx.x);
    else if (threadIdx.x >= 64 && threadIdx.x < 70) {
      const int k = (threadIdx.x - 64) >> 1, twin = (threadIdx.x - 64) & 1;      // [3 buffers][request, twin]
      amax[k * amax_stride + (twin ? B + b : b)] = pool_amax[(long)slot * 6 + (threadIdx.x - 64)];
    }
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;      // one f32x4 of a frame per thread
  const int t = (int)(idx / 20), q = (int)(idx - (long)t * 20);
  const long o = ((long)req[b].row + t) * 80 + 4 * q;
  if (t < len) {
    const long s = ((long)slot * Tcap + t) * 80 + 4 * q;
    *reinterpret_cast<f32x4*>(x + o) = *reinterpret_cast<const f32x4*>(pool_x + s);
    *reinterpret_cast<f32x4*>(mu + o) = *reinterpret_cast<const f32x4*>(pool_mu + s);
    *reinterpret_cast<f32x4*>(cond + o) = *reinterpret_cast<const f32x4*>(pool_cond + s);
  } else if (t < tfill) {      // uniform geometry: the padding up to the step's longest request is read (and masked) as rows
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(x + o) = z;
    *reinterpret_cast<f32x4*>(mu + o) = z;
    *reinterpret_cast<f32x4*>(cond + o) = z;
  }
}

int pool_gather(const PoolStepReq* req, int B, int tmax, int tfill, const float* pool_x, const float* pool_mu, const float* pool_cond,
                const float* pool_spks, const float* pool_amax, int Tcap, float* x, float* mu, float* cond, float* spks, float* amax,
                int amax_stride, hipStream_t st) {
  if (B <= 0 || tmax <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)cdivl((long)tmax * 20, 256), B), dim3(256), 0, st, req, B, tfill, pool_x,
                     pool_mu, pool_cond, pool_spks, pool_amax, Tcap, x, mu, cond, spks, amax, amax_stride);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// ---- Euler step with classifier-free guidance, a dt and a guidance rate per request (PoolStepReq::cfg), written back to the pool (rowops.hip euler_cfg_kernel's
// expressions), and the maxima the estimator's launches left in the request's and its twin's slots --------------------------------
__global__ __launch_bounds__(256) void pool_euler_scatter_kernel(const PoolStepReq* __restrict__ req, int B, const float* __restrict__ x,
                                                                 const float* __restrict__ d, const float* __restrict__ amax,
                                                                 int amax_stride, float* __restrict__ pool_x, float* __restrict__ pool_amax,
                                                                 int Tcap) {
  const int b = blockIdx.y;
  const int slot = req[b].slot, len = req[b].len;
  if (blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 70) {
    const int k = (threadIdx.x - 64) >> 1, twin = (threadIdx.x - 64) & 1;
    pool_amax[(long)slot * 6 + (threadIdx.x - 64)] = amax[k * amax_stride + (twin ? B + b : b)];
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = (int)(idx / 20), cc = (int)(idx - (long)t * 20) * 4;
  if (t >= len) return;
  const long r = (long)req[b].row + t, ru = (long)req[b].rowu + t;
  const float dt = req[b].dt, rate = req[b].cfg;
  const f32x4 dc = *reinterpret_cast<const f32x4*>(d + r * 80 + cc);
  const f32x4 du = *reinterpret_cast<const f32x4*>(d + ru * 80 + cc);
  f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * 80 + cc);
  const f32x4 g = (1.0f + rate) * dc - rate * du;
  xv = xv + dt * g;
  *reinterpret_cast<f32x4*>(pool_x + ((long)slot * Tcap + t) * 80 + cc) = xv;
}

int pool_euler_scatter(const PoolStepReq* req, int B, int tmax, const float* x, const float* d, const float* amax,
                       int amax_stride, float* pool_x, float* pool_amax, int Tcap, hipStream_t st) {
  if (B <= 0 || tmax <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_euler_scatter_kernel, dim3((unsigned)cdivl((long)tmax * 20, 256), B), dim3(256), 0, st, req, B, x, d,
                     amax, amax_stride, pool_x, pool_amax, Tcap);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// ---- a stage of a request's OWN solver (jv_cfm_pool_step_s; rowops.hip solver_stage_kernel's expressions) with the stage and its
// coefficient per request: requests on Euler, at a first and at a second stage share the launch.  pool_x always takes the estimator's
// next input, so pool_gather serves every stage; x0 / k1 of a request live in pool_x0 / pool_k1 under its slot ---------------------
__global__ __launch_bounds__(256) void pool_stage_scatter_kernel(const PoolStepReq* __restrict__ req, int B, const float* __restrict__ x,
                                                                 const float* __restrict__ d, const float* __restrict__ amax,
                                                                 int amax_stride, float* __restrict__ pool_x, float* __restrict__ pool_x0,
                                                                 float* __restrict__ pool_k1, float* __restrict__ pool_amax, int Tcap) {
  const int b = blockIdx.y;
  const int slot = req[b].slot, len = req[b].len, stage = req[b].stage;
  if (blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 70) {
    const int k = (threadIdx.x - 64) >> 1, twin = (threadIdx.x - 64) & 1;
    pool_amax[(long)slot * 6 + (threadIdx.x - 64)] = amax[k * amax_stride + (twin ? B + b : b)];
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = (int)(idx / 20), cc = (int)(idx - (long)t * 20) * 4;
  if (t >= len) return;
  const long r = (long)req[b].row + t, ru = (long)req[b].rowu + t;
  const float c = req[b].dt, rate = req[b].cfg;
  const f32x4 dc = *reinterpret_cast<const f32x4*>(d + r * 80 + cc);
  const f32x4 du = *reinterpret_cast<const f32x4*>(d + ru * 80 + cc);
  const f32x4 xin = *reinterpret_cast<const f32x4*>(x + r * 80 + cc);
  const f32x4 g = (1.0f + rate) * dc - rate * du;
  const long o = ((long)slot * Tcap + t) * 80 + cc;
  f32x4 base = xin, inc = g;
  if (stage & STAGE_SAVE_X0) *reinterpret_cast<f32x4*>(pool_x0 + o) = xin;
  if (stage & STAGE_SAVE_K1) *reinterpret_cast<f32x4*>(pool_k1 + o) = g;
  if (stage & STAGE_BASE_X0) base = *reinterpret_cast<const f32x4*>(pool_x0 + o);
  if (stage & STAGE_ADD_K1) inc = *reinterpret_cast<const f32x4*>(pool_k1 + o) + g;
  *reinterpret_cast<f32x4*>(pool_x + o) = base + c * inc;
}

int pool_stage_scatter(const PoolStepReq* req, int B, int tmax, const float* x, const float* d, const float* amax, int amax_stride,
                       float* pool_x, float* pool_x0, float* pool_k1, float* pool_amax, int Tcap, hipStream_t st) {
  if (B <= 0 || tmax <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_stage_scatter_kernel, dim3((unsigned)cdivl((long)tmax * 20, 256), B), dim3(256), 0, st, req, B, x, d,
                     amax, amax_stride, pool_x, pool_x0, pool_k1, pool_amax, Tcap);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// ---- fetch: frames first .. first + len - 1 of a slot to channels-first, zero-filled to Tm (rowops.hip rows_to_cf_from_kernel) ----
__global__ __launch_bounds__(256) void pool_fetch_kernel(const PoolFetchChunk ch, const float* __restrict__ pool_x, int Tcap,
                                                         float* __restrict__ mel, int Tm) {
  __shared__ float tile[32][33];
  const int i = blockIdx.z, b = ch.b0 + i, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int len = ch.r[i].len;
  const float* src = pool_x + ((long)ch.r[i].slot * Tcap + ch.r[i].first) * 80;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = t0 + ty + 8 * k, c = c0 + tx;
    tile[ty + 8 * k][tx] = (t < len && c < 80) ? src[(long)t * 80 + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, t = t0 + tx;
    if (c < 80 && t < Tm) mel[((long)b * 80 + c) * Tm + t] = tile[tx][ty + 8 * k];
  }
}

int pool_fetch(const PoolFetchChunk& ch, const float* pool_x, int Tcap, float* mel, int Tm, hipStream_t st) {
  if (ch.n <= 0 || Tm <= 0) return JV_OK;
  hipLaunchKernelGGL(pool_fetch_kernel, dim3(cdiv(Tm, 32), 3, ch.n), dim3(256), 0, st, ch, pool_x, Tcap, mel, Tm);
  JV_HIP(hipGetLastError());
  return JV_OK;
}

}  // namespace jv
