// dispatch.h -- runtime flags to template arguments (host only), for the launch code of quadenv.hip,
// rollout.hip and the actor files: f is a generic lambda that names its kernel with decltype(arg)::value.
#pragma once

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

}  // namespace quadenv
