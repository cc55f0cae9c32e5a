// dispatch.h -- runtime flags to template arguments (host only), for the launch code of quadenv.hip,
// rollout.hip and the actor files: f is a generic lambda that names its kernel with decltype(arg)::value.
// And the launch of the kernels that take more than 64 KB of dynamic LDS (lds_opt_in, launch_lds).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/quadenv.h"

namespace quadenv {

template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(mb): mb = H2 / 32 of a checked actor arch (2, 4 or 8: actor_core.h net_of admits no other)
template <class F>
auto with_mb(int mb, F&& f) {
  return mb == 2   ? f(std::integral_constant<int, 2>{})
         : mb == 4 ? f(std::integral_constant<int, 4>{})
                   : f(std::integral_constant<int, 8>{});
}

// f(kind, flag): kind = QUAD_ENV_TRAJ / QUAD_ENV_HOVER, flag = the kernel family's second argument
template <class F>
auto with_kind(bool traj, bool flag, F&& f) {
  return with_bool(flag, [&](auto fl) {
    return traj ? f(std::integral_constant<int, QUAD_ENV_TRAJ>{}, fl)
                : f(std::integral_constant<int, QUAD_ENV_HOVER>{}, fl);
  });
}

// A kernel that takes more than 64 KB of dynamic LDS (gfx950 has 160 KB per CU) must be opted in, per kernel
// and per device. KERNEL is the kernel itself (&k<..>), not its type, so every instantiation has a table of its
// own: kernels of one signature would share a table keyed on the type, and only the first would be opted in.
// Several kernels (policy.hip's three) are opted in together, under one table and one hipGetDevice.
// The one rule: hipGetDevice failing is the caller's error; a device index outside the table is not cached and
// opts in on every call.
template <auto... KERNEL>
hipError_t lds_opt_in(int bytes) {
  static bool opted[64] = {};
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev)) return e;
  const bool cached = dev >= 0 && dev < 64;
  if (cached && opted[dev]) return hipSuccess;
  hipError_t e = hipSuccess;
  ((e = e != hipSuccess ? e
                        : hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, bytes)),
   ...);
  if (e == hipSuccess && cached) opted[dev] = true;
  return e;
}

// opt in, launch, and the launch's error
template <auto KERNEL, class... A>
hipError_t launch_lds(dim3 grid, dim3 block, int bytes, hipStream_t s, A... args) {
  if (const hipError_t e = lds_opt_in<KERNEL>(bytes)) return e;
  hipLaunchKernelGGL(KERNEL, grid, block, bytes, s, args...);
  return hipGetLastError();
}

}  // namespace quadenv
