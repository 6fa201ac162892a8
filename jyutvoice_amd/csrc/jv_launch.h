// Host-side launch helpers of the row-owning kernels (rowgemm.hip, rowblock.hip, hiftconv.hip).
#pragma once
#include <type_traits>

#include "jv_common.h"

namespace jv {

// One launch of `Kernel` (an instantiation, named as the template argument: each has its own record below) with `lds` bytes
// of dynamic LDS:
//   * hipFuncAttributeMaxDynamicSharedMemorySize is raised when this device has not yet seen an LDS size that large for
//     this kernel (the attribute belongs to the kernel's image on the current device; a kernel with one fixed size raises
//     it once, one whose size depends on the arguments whenever a larger one comes along);
//   * with the profiler on, the launch is bracketed by its events: `prof_done` calls prof_end(st, name, flops, bytes) with
//     the launch's profiler name and its algorithmic work;
//   * the result is hipGetLastError's.
template <auto Kernel, class Args, class ProfDone>
int launch_lds(const dim3 grid, const dim3 block, const int lds, hipStream_t st, const Args& a, ProfDone&& prof_done) {
  static int raised[64] = {};      // per device: the LDS size the attribute was last raised to
  int dev = 0;
  JV_HIP(hipGetDevice(&dev));
  if (raised[dev & 63] < lds) {
    JV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    raised[dev & 63] = lds;
  }
  const bool prof = prof_on();
  if (prof) prof_begin(st);
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, a);
  if (prof) prof_done();
  JV_HIP(hipGetLastError());
  return JV_OK;
}

// tile height rt = 2 .. 5 (in 16-row units) -> f(std::integral_constant<int, RT>{}); any other value fails with `what`
template <class F>
int dispatch_rt(const int rt, const char* what, F&& f) {
  switch (rt) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    default: return fail(JV_ERR_ARG, what);
  }
}

}  // namespace jv
