// actor_arch.hip -- the general deterministic actor (actor_arch.h: 12 -> H1 -> H2 -> 4, ReLU or tanh) behind
// quad_actor_pack / quad_actor_act, and the fused episode and waypoint-lap kernels that fly it
// (quad_actor_episode / quad_actor_waypoints): policy_episode_body.h's closed loop with actor_arch.h's forward
// in the 128 net's place.
//
// Kernels
//   actor::k_pack<arch::Layout, ..>     torch [out, in] parameters -> the packed image (actor_arch.h's layout)
//   k_actor_act<MB>                     mean and clip(mean) of n rows, one wave per 32-row tile, grid-stride
//   k_actor_episode<KIND, CTBR, MODE, MB>, k_actor_waypoints<CTBR, MODE, MB>
//                                       episode_body<.., NT = 1, EB = 64, ..> (64-env blocks of two one-tile
//                                       waves), the handle's constant block read from memory (no SPEC form)
//   k_pop_actor_episode<KIND, CTBR, MODE, MB>  k_actor_episode behind the population's grid dimension
//
// This file is compiled once without AA_KIND (every quad_actor_* entry point, the pack kernel, k_actor_act, the
// launch dispatch) and once per (AA_KIND, AA_MB): AA_KIND = 0 hover / 1 trajectory / 2 hover waypoint laps, AA_MB =
// H2 / 32 = 2 / 4 / 8 -- nine objects of four kernels each that build in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "actor_arch.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "handle.h"
#include "policy_episode.h"
#include "policy_episode_body.h"
#include "population.h"

namespace quadenv {

// one (kind, MB) object's instantiations, defined and explicitly instantiated in that object; wr is read by the
// waypoint kind only
template <int AKIND, int MB>
hipError_t launch_actor_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode, const ActorNet& net,
                             const float* packed, const EpisodeArgs& a, const QuadWaypointRun* wr, hipStream_t s);
template <int AKIND, int MB>  // (the episode kinds, 0 and 1)
hipError_t launch_pop_actor_inst(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active, int count,
                                 int n, bool ctbr, int obs_mode, const ActorNet& net, hipStream_t s);

#if defined(AA_KIND)
namespace {

// actor_arch.h's forward as episode_body's forward (policy_episode_body.h)
template <int MB>
struct ArchForward {
  const float* __restrict__ packed;
  actor::Net net;
  template <int BLK>
  __device__ __forceinline__ void stage() {
    extern __shared__ float lds[];
    actor::stage<BLK>(lds, packed, arch::Layout{net.nb1, MB}.lds_floats());
  }
  __device__ __forceinline__ void operator()(const float (&ob)[12], float (&act)[ACT]) const {
    extern __shared__ float lds[];
    float xb[1][8];
    fragments<1>(ob, xb);
    arch::forward<MB>(lds, packed, net, xb[0], act);  // quad_actor_act's mean
  }
};

#if AA_KIND == 2
template <bool CTBR, int MODE, int MB>
__global__ __launch_bounds__(128) void k_actor_waypoints(const KConsts<float>* __restrict__ kc, KParams p,
                                                         const float* __restrict__ packed, actor::Net net,
                                                         EpisodeArgs a, QuadWaypointRun wr) {
  p.kc = kc;
  ArchForward<MB> fw{packed, net};
  episode_body<QUAD_ENV_HOVER, CTBR, 1, MODE, 64, true>(*kc, p, fw, a, &wr);
}
#else
template <int KIND, bool CTBR, int MODE, int MB>
__global__ __launch_bounds__(128) void k_actor_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                       const float* __restrict__ packed, actor::Net net,
                                                       EpisodeArgs a) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  ArchForward<MB> fw{packed, net};
  episode_body<KIND, CTBR, 1, MODE, 64, false>(*kc, p, fw, a, nullptr);
}

// The population form (quad_pop_episode of a population of this family), in k_actor_episode's two observation modes
// (QUAD_OBS_DEPLOYED: a quad_pop_create_deployed population); the member's entry is read through
// pop::const_entry (population.h), its image the policy half of the member's actor-critic image
template <int KIND, bool CTBR, int MODE, int MB>
__global__ __launch_bounds__(128) void k_pop_actor_episode(const KConsts<float>* __restrict__ kc,
                                                           const PopEpisodeEntry* __restrict__ tab,
                                                           const int32_t* __restrict__ active, actor::Net net) {
#if defined(__HIP_DEVICE_COMPILE__)  // (pop::const_entry, population.h)
  const auto& en = pop::const_entry(tab, active[blockIdx.y]);
  KParams p = en.kp;
  p.kc = kc;
  const EpisodeArgs a = en.a;
  ArchForward<MB> fw{en.packed, net};
  episode_body<KIND, CTBR, 1, MODE, 64, false>(*kc, p, fw, a, nullptr);
#endif
}
#endif

}  // namespace

#if AA_KIND != 2
template <int AKIND, int MB>
hipError_t launch_pop_actor_inst(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active, int count,
                                 int n, bool ctbr, int obs_mode, const ActorNet& net, hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  const int bytes = arch::Layout{net.nb1, MB}.lds_bytes();  // <= 64 KB: no opt-in
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(obs_mode == QUAD_OBS_DEPLOYED, [&](auto dm) {
      constexpr bool CB = decltype(cb)::value;
      constexpr int MD = decltype(dm)::value ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV;
      hipLaunchKernelGGL((k_pop_actor_episode<AKIND, CB, MD, MB>), dim3((n + 63) / 64, count), dim3(128), bytes, s, kc,
                         tab, active, dn);
      return hipGetLastError();
    });
  });
}
template hipError_t launch_pop_actor_inst<AA_KIND, AA_MB>(const KConsts<float>*, const PopEpisodeEntry*, const int32_t*,
                                                          int, int, bool, int, const ActorNet&, hipStream_t);
#endif

template <int AKIND, int MB>
hipError_t launch_actor_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode, const ActorNet& net,
                             const float* packed, const EpisodeArgs& a, const QuadWaypointRun* wr, hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  const int bytes = arch::Layout{net.nb1, MB}.lds_bytes();  // <= 64 KB: no opt-in
  const dim3 grid((kp.n + 63) / 64), block(128);
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(obs_mode == QUAD_OBS_DEPLOYED, [&](auto dm) {
      constexpr bool CB = decltype(cb)::value;
      constexpr int MD = decltype(dm)::value ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV;
#if AA_KIND == 2
      hipLaunchKernelGGL((k_actor_waypoints<CB, MD, MB>), grid, block, bytes, s, kc, kp, packed, dn, a, *wr);
#else
      hipLaunchKernelGGL((k_actor_episode<AKIND, CB, MD, MB>), grid, block, bytes, s, kc, kp, packed, dn, a);
#endif
      return hipGetLastError();
    });
  });
}
template hipError_t launch_actor_inst<AA_KIND, AA_MB>(const KConsts<float>*, const KParams&, bool, int, const ActorNet&,
                                                      const float*, const EpisodeArgs&, const QuadWaypointRun*,
                                                      hipStream_t);

}  // namespace quadenv

#else  // the C entry points' object

namespace {

int afail(int code, const char* m) { return set_error(code, m); }

template <int AKIND>
hipError_t launch_by_mb(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode, const ActorNet& net,
                        const float* packed, const EpisodeArgs& a, const QuadWaypointRun* wr, hipStream_t s) {
  return with_mb(net.mb, [&](auto mb) {
    return launch_actor_inst<AKIND, decltype(mb)::value>(kc, kp, ctbr, obs_mode, net, packed, a, wr, s);
  });
}

// ---- act (actor_core.h act_tiles): mean and clip(mean) of a row
template <int MB>
__global__ __launch_bounds__(actor::ACT_BLK) void k_actor_act(const float* __restrict__ packed, actor::Net net,
                                                              const float* __restrict__ obs, float* __restrict__ mean,
                                                              float* __restrict__ actions_env, int32_t n) {
  extern __shared__ float lds[];
  actor::stage<actor::ACT_BLK>(lds, packed, arch::Layout{net.nb1, MB}.lds_floats());
  actor::act_tiles(n, [&](int row, bool ok, int h) {
    float xb[8], out[ACT];
#pragma unroll
    for (int k = 0; k < 8; k++) xb[k] = ok && (h == 0 || k < 4) ? obs[size_t(row) * OBS + 8 * h + k] : 0.f;
    arch::forward<MB>(lds, packed, net, xb, out);
    if (!ok || h) return;  // one lane per row stores
    if (mean) {
#pragma unroll
      for (int k = 0; k < ACT; k++) mean[size_t(row) * ACT + k] = out[k];
    }
    reinterpret_cast<float4*>(actions_env)[row] =
        make_float4(fminf(fmaxf(out[0], -1.f), 1.f), fminf(fmaxf(out[1], -1.f), 1.f),
                    fminf(fmaxf(out[2], -1.f), 1.f), fminf(fmaxf(out[3], -1.f), 1.f));
  });
}

// QUAD_OK and *out, or QUAD_EINVAL with a message for an arch outside the family
int actor_net_of(const QuadActorArch* a, ActorNet* out) { return actor::net_of(a, "actor arch", false, out); }

}  // namespace

// the population form of quad_actor_episode (population.h); `arch` is one quad_pop_create_arch checked
hipError_t pop::launch_pop_actor_episode(const QuadActorArch& arch, const KConsts<float>* kc, const PopEpisodeEntry* tab,
                                         const int32_t* active, int count, int n, int env_kind, bool ctbr,
                                         int obs_mode, hipStream_t s) {
  const ActorNet net{arch.h1 / 32, arch.h2 / 32, arch.activation};
  return with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    return env_kind == QUAD_ENV_TRAJ ? launch_pop_actor_inst<1, MB>(kc, tab, active, count, n, ctbr, obs_mode, net, s)
                                     : launch_pop_actor_inst<0, MB>(kc, tab, active, count, n, ctbr, obs_mode, net, s);
  });
}

}  // namespace quadenv

using namespace quadenv;

extern "C" {

int64_t quad_actor_packed_floats(const QuadActorArch* a) {
  ActorNet net;
  if (actor_net_of(a, &net)) return -1;
  return arch::Layout{net.nb1, net.mb}.floats();
}

int quad_actor_pack(const QuadActorArch* a, const QuadActorParams* p, float* packed, void* stream) {
  ActorNet net;
  if (int rc = actor_net_of(a, &net)) return rc;
  if (!p || !packed) return afail(QUAD_EINVAL, "quad_actor_pack: params/packed is NULL");
  if (!p->w0 || !p->b0 || !p->w1 || !p->b1 || !p->w2 || !p->b2)
    return afail(QUAD_EINVAL, "quad_actor_pack: a parameter pointer is NULL");
  if (reinterpret_cast<uintptr_t>(packed) & 15u) return afail(QUAD_EINVAL, "quad_actor_pack: packed must be 16-byte aligned");
  const hipError_t e = actor::launch_pack<arch::Layout, true, OBS>(arch::Layout{net.nb1, net.mb}, *p, packed,
                                                                  static_cast<hipStream_t>(stream));
  return e == hipSuccess ? QUAD_OK : afail(QUAD_EHIP, "k_actor_pack launch failed");
}

int quad_actor_act(const QuadActorArch* a, const float* packed, const float* obs, float* mean, float* actions_env,
                   int32_t n, void* stream) {
  ActorNet net;
  if (int rc = actor_net_of(a, &net)) return rc;
  if (!packed || !obs || !actions_env) return afail(QUAD_EINVAL, "quad_actor_act: NULL argument");
  if (n <= 0) return afail(QUAD_EINVAL, "quad_actor_act: n must be > 0");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(actions_env)) & 15u)
    return afail(QUAD_EINVAL, "quad_actor_act: packed and actions_env must be 16-byte aligned");
  const hipError_t e = with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const int bytes = arch::Layout{net.nb1, MB}.lds_bytes();
    hipLaunchKernelGGL((k_actor_act<MB>), actor::act_grid(n), dim3(actor::ACT_BLK), bytes,
                       static_cast<hipStream_t>(stream), packed, actor::Net{net.nb1, net.actfn}, obs, mean, actions_env, n);
    return hipGetLastError();
  });
  return e == hipSuccess ? QUAD_OK : afail(QUAD_EHIP, "k_actor_act launch failed");
}

// ---- the episode and the laps: quad_policy_episode's / quad_policy_waypoints' checks and arguments
int quad_actor_episode(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadPolicyRun* r,
                       void* stream) {
  ActorNet net;
  if (int rc = actor_net_of(arch, &net)) return rc;
  EpisodeArgs a{};
  if (int rc = pop::episode_args(h, packed, r, &a, "quad_actor_episode")) return rc;
  DeviceGuard g(h->device);
  const bool ctbr = h->cfg.wrapper == QUAD_WRAP_CTBR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h->cfg.env_kind == QUAD_ENV_TRAJ ? launch_by_mb<1>(h->kdev, h->kp, ctbr, r->obs_mode, net, packed, a, nullptr, s)
                                           : launch_by_mb<0>(h->kdev, h->kp, ctbr, r->obs_mode, net, packed, a, nullptr, s));
  return QUAD_OK;
}

int quad_actor_waypoints(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadPolicyRun* r,
                         const QuadWaypointRun* wr, void* stream) {
  ActorNet net;
  if (int rc = actor_net_of(arch, &net)) return rc;
  EpisodeArgs a{};
  if (int rc = waypoints_args(h, packed, r, wr, &a, "quad_actor_waypoints")) return rc;
  DeviceGuard g(h->device);
  HIP_TRY(launch_by_mb<2>(h->kdev, h->kp, h->cfg.wrapper == QUAD_WRAP_CTBR, r->obs_mode, net, packed, a, wr,
                          static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

}  // extern "C"
#endif
