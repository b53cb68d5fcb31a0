// pbs_launch.hpp — the host side of a fused PBS kernel launch, shared by pbs.hip, pbs1024_quad.hip,
// pbs1024_hex.hip, pbs2048.hip, pbs1024k2.hip, pbs_small.hip and pbs512k4.hip.
#pragma once
#include "common.hpp"
#include "fft512.hpp"
#include "pbs.hpp"

#include <type_traits>

namespace chip {

// what every fused launcher answers to a parameter set outside its gate
inline int reject_params(const PbsArgs& a) {
  set_error("unsupported PBS parameters: N=%u k=%u level=%u base_log=%u limbs=%u", a.N, a.k, a.level, a.base_log,
            a.limbs);
  return -2;
}

// f(std::true_type) when the caller asked for the rounding residual (the kernels' RESID builds), else
// f(std::false_type)
template <class F>
int with_resid(const PbsArgs& a, F&& f) {
  return a.resid ? f(std::true_type{}) : f(std::false_type{});
}

// Launches `kern` on ceil(num_samples / cts) workgroups of `threads` threads with `lds` bytes of
// dynamic LDS.  Every fused kernel takes (out, out_idx, luts, lut_idx, in, in_idx, fbsk, n, base_log,
// num_samples, resid, guard); the kernels that run one level at a time take the level count after n.
template <class... KArgs>
int launch_fused(void (*kern)(KArgs...), int cts, int threads, size_t lds, const PbsArgs& a) {
  static_assert(sizeof...(KArgs) == 12 || sizeof...(KArgs) == 13, "a fused PBS kernel's arguments");
  CHIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const uint32_t blocks = (a.num_samples + cts - 1) / cts;
  const cplx* fbsk = reinterpret_cast<const cplx*>(a.fbsk);
  if constexpr (sizeof...(KArgs) == 13) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, a.stream, a.out, a.out_idx, a.luts, a.lut_idx, a.in,
                       a.in_idx, fbsk, a.n, a.level, a.base_log, a.num_samples, a.resid, a.guard);
  } else {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, a.stream, a.out, a.out_idx, a.luts, a.lut_idx, a.in,
                       a.in_idx, fbsk, a.n, a.base_log, a.num_samples, a.resid, a.guard);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("pbs launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace chip
