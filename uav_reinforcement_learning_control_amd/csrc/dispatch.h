// dispatch.h -- runtime flags to template arguments (host only), for the launch code of quadenv.hip and
// rollout.hip: f is a generic lambda that names its kernel with decltype(arg)::value.
#pragma once

#include <type_traits>

#include "../../include/quadenv.h"

namespace quadenv {

template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
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
