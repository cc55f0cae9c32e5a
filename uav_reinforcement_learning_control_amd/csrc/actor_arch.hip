// actor_arch.hip -- the general deterministic actor (actor_arch.h: 12 -> H1 -> H2 -> 4, ReLU or tanh) behind
// quad_actor_pack / quad_actor_act, and the fused episode and waypoint-lap kernels that fly it
// (quad_actor_episode / quad_actor_waypoints): policy_episode_body.h's closed loop with actor_arch.h's forward
// in the 128 net's place.
//
// Kernels
//   k_actor_pack                        torch [out, in] parameters -> the packed image (actor_arch.h's layout)
//   k_actor_act<MB>                     mean and clip(mean) of n rows, one wave per 32-row tile, grid-stride
//   k_actor_episode<KIND, CTBR, MODE, MB>, k_actor_waypoints<CTBR, MODE, MB>
//                                       episode_body<.., NT = 1, EB = 64, ..> (64-env blocks of two one-tile
//                                       waves), the handle's constant block read from memory (no SPEC form)
//
// This file is compiled once without AA_KIND (the C entry points, k_actor_pack, k_actor_act, the launch
// dispatch) and once per (AA_KIND, AA_MB): AA_KIND = 0 hover / 1 trajectory / 2 hover waypoint laps, AA_MB =
// H2 / 32 = 2 / 4 / 8 -- nine objects of four kernels each that build in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "actor_arch.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "policy_episode.h"
#include "policy_episode_body.h"

namespace quadenv {

int set_error(int code, const char* msg);  // quadenv.hip

// one (kind, MB) object's instantiations; wr is read by the waypoint kind only
template <int AKIND, int MB>
hipError_t launch_actor_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode, const ActorNet& net,
                             const float* packed, const EpisodeArgs& a, const QuadWaypointRun* wr, hipStream_t s);

#if defined(AA_KIND)
namespace {

// actor_arch.h's forward as episode_body's forward (policy_episode_body.h)
template <int MB>
struct ArchForward {
  const float* __restrict__ packed;
  arch::Net net;
  template <int BLK>
  __device__ __forceinline__ void stage() {
    extern __shared__ float lds[];
    arch::stage<BLK>(lds, packed, arch::Layout{net.nb1, MB});
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
                                                         const float* __restrict__ packed, arch::Net net,
                                                         EpisodeArgs a, QuadWaypointRun wr) {
  p.kc = kc;
  ArchForward<MB> fw{packed, net};
  episode_body<QUAD_ENV_HOVER, CTBR, 1, MODE, 64, true>(*kc, p, fw, a, &wr);
}
#else
template <int KIND, bool CTBR, int MODE, int MB>
__global__ __launch_bounds__(128) void k_actor_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                       const float* __restrict__ packed, arch::Net net,
                                                       EpisodeArgs a) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  ArchForward<MB> fw{packed, net};
  episode_body<KIND, CTBR, 1, MODE, 64, false>(*kc, p, fw, a, nullptr);
}
#endif

}  // namespace

template <>
hipError_t launch_actor_inst<AA_KIND, AA_MB>(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode,
                                             const ActorNet& net, const float* packed, const EpisodeArgs& a,
                                             const QuadWaypointRun* wr, hipStream_t s) {
  const arch::Net dn{net.nb1, net.tanh_act};
  const int bytes = arch::Layout{net.nb1, AA_MB}.lds_floats() * int(sizeof(float));  // <= 64 KB: no opt-in
  const dim3 grid((kp.n + 63) / 64), block(128);
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(obs_mode == QUAD_OBS_DEPLOYED, [&](auto dm) {
      constexpr bool CB = decltype(cb)::value;
      constexpr int MD = decltype(dm)::value ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV;
#if AA_KIND == 2
      hipLaunchKernelGGL((k_actor_waypoints<CB, MD, AA_MB>), grid, block, bytes, s, kc, kp, packed, dn, a, *wr);
#else
      hipLaunchKernelGGL((k_actor_episode<AA_KIND, CB, MD, AA_MB>), grid, block, bytes, s, kc, kp, packed, dn, a);
#endif
      return hipGetLastError();
    });
  });
}

}  // namespace quadenv

#else  // the C entry points' object

#define AA_DECLARE(K, M)                                                                                          \
  template <>                                                                                                     \
  hipError_t launch_actor_inst<K, M>(const KConsts<float>*, const KParams&, bool, int, const ActorNet&, const float*, \
                                     const EpisodeArgs&, const QuadWaypointRun*, hipStream_t);
AA_DECLARE(0, 2) AA_DECLARE(0, 4) AA_DECLARE(0, 8)
AA_DECLARE(1, 2) AA_DECLARE(1, 4) AA_DECLARE(1, 8)
AA_DECLARE(2, 2) AA_DECLARE(2, 4) AA_DECLARE(2, 8)
#undef AA_DECLARE

namespace {

int afail(int code, const char* m) { return set_error(code, m); }

template <int AKIND>
hipError_t launch_by_mb(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode, const ActorNet& net,
                        const float* packed, const EpisodeArgs& a, const QuadWaypointRun* wr, hipStream_t s) {
  switch (net.mb) {
    case 2: return launch_actor_inst<AKIND, 2>(kc, kp, ctbr, obs_mode, net, packed, a, wr, s);
    case 4: return launch_actor_inst<AKIND, 4>(kc, kp, ctbr, obs_mode, net, packed, a, wr, s);
    case 8: return launch_actor_inst<AKIND, 8>(kc, kp, ctbr, obs_mode, net, packed, a, wr, s);
  }
  return hipErrorInvalidValue;  // actor_net_of admits no other
}

// ---- pack: one thread per float of the f32 regions, then one per (block n, lane) unit of the W1 pieces and
// one per (k-step g, lane) unit of the W2 pieces
__global__ void k_actor_pack(QuadActorParams p, int h1, int h2, float* __restrict__ out) {
  const arch::Layout lay{h1 / 32, h2 / 32};
  const int nf = lay.w1p(), n1 = lay.nb1 * 64, n2 = lay.steps() * 64;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nf + n1 + n2) return;
  if (idx < nf) {
    float v;
    if (idx < lay.w3()) {  // B1 | B2: [block][half][reg]
      const bool second = idx >= lay.b2();
      const int t = idx - (second ? lay.b2() : 0);
      v = (second ? p.b1 : p.b0)[32 * (t / 32) + acc_row(t % 16, (t / 16) % 2)];
    } else if (idx < lay.b3()) {  // W3: [m][reg][half][out]
      const int t = idx - lay.w3();
      v = p.w2[(t % 4) * h2 + 32 * (t / 128) + acc_row((t / 8) % 16, (t / 4) % 2)];
    } else {
      v = p.b2[idx - lay.b3()];
    }
    out[idx] = v;
    return;
  }
  const int u = idx - nf;
  const int lane = u % 64, r = lane & 31, h = lane >> 5;
  float v8[8];
  bf16x8* dst;
  if (u < n1) {  // A[neuron 32 n + r][feature 8 h + j]
    const int n = u / 64;
#pragma unroll
    for (int j = 0; j < 8; j++) v8[j] = 8 * h + j < OBS ? p.w0[(32 * n + r) * OBS + 8 * h + j] : 0.f;
    dst = reinterpret_cast<bf16x8*>(out + lay.w1p()) + n * 3 * 64 + lane;
  } else {  // A[neuron 32 m + r][input 32 n + acc_row(8 t + j, h)] of k-step g = (n * 2 + t) * MB + m
    const int g = (u - n1) / 64, m = g % lay.mb, t = (g / lay.mb) % 2, n = g / (2 * lay.mb);
#pragma unroll
    for (int j = 0; j < 8; j++) v8[j] = p.w1[size_t(32 * m + r) * h1 + 32 * n + acc_row(8 * t + j, h)];
    dst = reinterpret_cast<bf16x8*>(out + lay.w2p()) + g * 3 * 64 + lane;
  }
  const P3 x = split8(v8);
#pragma unroll
  for (int q = 0; q < 3; q++) dst[q * 64] = x.p[q];
}

// ---- act: wave w of the grid takes the 32-row tiles w, w + waves, ...; lanes l and l + 32 carry row l & 31
constexpr int ACT_BLK = 256;
template <int MB>
__global__ __launch_bounds__(ACT_BLK) void k_actor_act(const float* __restrict__ packed, arch::Net net,
                                                       const float* __restrict__ obs, float* __restrict__ mean,
                                                       float* __restrict__ actions_env, int32_t n) {
  extern __shared__ float lds[];
  arch::stage<ACT_BLK>(lds, packed, arch::Layout{net.nb1, MB});
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5;
  const int tiles = (n + TILE - 1) / TILE;
  for (int tile = blockIdx.x * (ACT_BLK / 64) + wave; tile < tiles; tile += gridDim.x * (ACT_BLK / 64)) {
    const int row = tile * TILE + (lane & 31);
    const bool ok = row < n;
    float xb[8], out[ACT];
#pragma unroll
    for (int k = 0; k < 8; k++) xb[k] = ok && (h == 0 || k < 4) ? obs[size_t(row) * OBS + 8 * h + k] : 0.f;
    arch::forward<MB>(lds, packed, net, xb, out);
    if (!ok || h) continue;  // one lane per row stores
    if (mean) {
#pragma unroll
      for (int k = 0; k < ACT; k++) mean[size_t(row) * ACT + k] = out[k];
    }
    reinterpret_cast<float4*>(actions_env)[row] =
        make_float4(fminf(fmaxf(out[0], -1.f), 1.f), fminf(fmaxf(out[1], -1.f), 1.f),
                    fminf(fmaxf(out[2], -1.f), 1.f), fminf(fmaxf(out[3], -1.f), 1.f));
  }
}

template <int MB>
hipError_t launch_act(const ActorNet& net, const float* packed, const float* obs, float* mean, float* actions_env,
                      int32_t n, hipStream_t s) {
  const int tiles = (n + TILE - 1) / TILE, want = (tiles + ACT_BLK / 64 - 1) / (ACT_BLK / 64);
  const int bytes = arch::Layout{net.nb1, MB}.lds_floats() * int(sizeof(float));
  hipLaunchKernelGGL((k_actor_act<MB>), dim3(want < 512 ? want : 512), dim3(ACT_BLK), bytes, s, packed,
                     arch::Net{net.nb1, net.tanh_act}, obs, mean, actions_env, n);
  return hipGetLastError();
}

}  // namespace

int actor_net_of(const QuadActorArch* a, ActorNet* out) {
  if (!a) return afail(QUAD_EINVAL, "actor arch is NULL");
  if (a->h1 < 32 || a->h1 > arch::MAX_H1 || a->h1 % 32 != 0)
    return afail(QUAD_EINVAL, "actor arch: h1 must be a multiple of 32 in [32, 512]");
  if (a->h2 != 64 && a->h2 != 128 && a->h2 != 256) return afail(QUAD_EINVAL, "actor arch: h2 must be 64, 128 or 256");
  if (a->activation != QUAD_ACTFN_RELU && a->activation != QUAD_ACTFN_TANH)
    return afail(QUAD_EINVAL, "actor arch: activation must be QUAD_ACTFN_RELU or QUAD_ACTFN_TANH");
  *out = ActorNet{a->h1 / 32, a->h2 / 32, a->activation == QUAD_ACTFN_TANH ? 1 : 0};
  return QUAD_OK;
}

hipError_t launch_actor_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool ctbr, int obs_mode,
                                const ActorNet& net, const float* packed, const EpisodeArgs& a, hipStream_t s) {
  return env_kind == QUAD_ENV_TRAJ ? launch_by_mb<1>(kc, kp, ctbr, obs_mode, net, packed, a, nullptr, s)
                                   : launch_by_mb<0>(kc, kp, ctbr, obs_mode, net, packed, a, nullptr, s);
}

hipError_t launch_actor_waypoints(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode,
                                  const ActorNet& net, const float* packed, const EpisodeArgs& a,
                                  const QuadWaypointRun& wr, hipStream_t s) {
  return launch_by_mb<2>(kc, kp, ctbr, obs_mode, net, packed, a, &wr, s);
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
  const arch::Layout lay{net.nb1, net.mb};
  const int threads = lay.w1p() + lay.nb1 * 64 + lay.steps() * 64;
  hipLaunchKernelGGL(k_actor_pack, dim3((threads + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), *p,
                     a->h1, a->h2, packed);
  return hipGetLastError() == hipSuccess ? QUAD_OK : afail(QUAD_EHIP, "k_actor_pack launch failed");
}

int quad_actor_act(const QuadActorArch* a, const float* packed, const float* obs, float* mean, float* actions_env,
                   int32_t n, void* stream) {
  ActorNet net;
  if (int rc = actor_net_of(a, &net)) return rc;
  if (!packed || !obs || !actions_env) return afail(QUAD_EINVAL, "quad_actor_act: NULL argument");
  if (n <= 0) return afail(QUAD_EINVAL, "quad_actor_act: n must be > 0");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(actions_env)) & 15u)
    return afail(QUAD_EINVAL, "quad_actor_act: packed and actions_env must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = net.mb == 2   ? launch_act<2>(net, packed, obs, mean, actions_env, n, s)
                       : net.mb == 4 ? launch_act<4>(net, packed, obs, mean, actions_env, n, s)
                                     : launch_act<8>(net, packed, obs, mean, actions_env, n, s);
  return e == hipSuccess ? QUAD_OK : afail(QUAD_EHIP, "k_actor_act launch failed");
}

}  // extern "C"
#endif
