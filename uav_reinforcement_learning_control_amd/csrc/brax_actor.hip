// brax_actor.hip -- the Brax-profile policy (brax_actor.h: 21 -> H1 -> H2 -> 8, ReLU / tanh / SiLU, the running
// statistics' normaliser in front) behind quad_brax_actor_pack / quad_brax_actor_act / quad_brax_actor_sample, and the
// fused episode kernel of the brax env kinds that flies it (quad_brax_episode). The learner's unroll kernel
// (quad_brax_unroll: the entry point is here, beside quad_brax_episode) is brax_unroll.hip.
//
// Kernels
//   actor::k_pack<brax::Layout, ..>
//                             flax [in, out] parameters + mean / std / min_std -> the packed image
//   k_brax_act<MB, SAMPLE>    logits and the env action of n rows, one wave per 32-row tile, grid-stride; SAMPLE: the
//                             sampled action with its raw value and log-prob
//   k_brax_episode<KIND, MB>  whole episodes: 64-env blocks of two one-tile waves, every env's state in registers,
//                             per step forward -> NormalTanh -> brax_step -> metrics; the handle's constant block
//                             is read from memory
//
// Two rules keep the launch bit-identical to quad_brax_actor_act + quad_step per step: the forward and the action
// draw are brax_actor.h's one definition, executed by the full wave outside every per-lane branch; and this file is
// built with quadenv.o's floating-point flags (-ffp-contract=on, no SLP vectorizer), so brax_step has k_step_brax's
// bits.
//
// This file is compiled once without BA_KIND (every quad_brax_* entry point, the pack kernel, k_brax_act, the launch dispatch) and
// once per (BA_KIND, BA_MB): BA_KIND = 0 brax hover / 1 brax trajectory, BA_MB = H2 / 32 = 2 / 4 / 8.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "brax_actor.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "handle.h"
#include "quad_physics.h"

namespace quadenv {

#if defined(BA_KIND)
namespace {

// Has this env's episode ended already? brax_step's own tests on the state in hand: a step count above zero (a
// reset state has flown no step, whatever its position) and the kind's done predicate, or the EpisodeWrapper limit.
template <int KIND>
__device__ __forceinline__ int32_t entry_status(const KConsts<float>& k, const EnvRegs<float>& e) {
  if (e.step <= 0) return QUAD_PID_RUNNING;
  const float pos[3] = {e.pos[0], e.pos[1], e.pos[2]};
  const bool oxy = q_abs(pos[0]) > k.term_hi[0] || q_abs(pos[1]) > k.term_hi[1];
  const bool oz = pos[2] < k.term_lo[2] || pos[2] > k.term_hi[2];
  bool term = oxy || oz;
  if (KIND == QUAD_ENV_BRAX_TRAJ) {
    bool fin = true, ov = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      fin &= q_abs(e.pos[i]) <= 3.4028235e38f && q_abs(e.v[i]) <= 3.4028235e38f && q_abs(e.w[i]) <= 3.4028235e38f;
      ov |= q_abs(e.v[i]) > k.bx_vlim;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
      fin &= q_abs(e.q[i]) <= 3.4028235e38f && q_abs(e.th[i]) <= 3.4028235e38f && q_abs(e.s[i]) <= 3.4028235e38f;
    term = !(fin && !oxy && !oz && !ov);
  }
  if (term) return QUAD_PID_TERMINATED;
  return e.step >= k.max_steps ? QUAD_PID_TRUNCATED : QUAD_PID_RUNNING;
}

template <int KIND, int MB>
__global__ __launch_bounds__(128) void k_brax_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                      const float* __restrict__ packed, actor::Net net,
                                                      BraxEpisodeArgs a) {
  extern __shared__ float lds[];
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  const KConsts<float>& K = *kc;
  const brax::Layout lay{net.nb1, MB};
  const int w = threadIdx.x >> 6;
  const bool h = (threadIdx.x & 32) != 0;
  const int i_raw = blockIdx.x * 64 + w * 32 + int(threadIdx.x & 31);
  const bool ok = i_raw < p.n;
  const bool owner = ok && !h;  // lanes l and l + 32 carry env l & 31 (the same bits); the lower half stores
  // lanes past the last env shadow it (in-range loads, MFMA columns of their own) and store nothing
  const int i = ok ? i_raw : p.n - 1;

  EnvRegs<float> e;
  load_env(p, i, e, true);
  actor::stage<128>(lds, packed, lay.lds_floats());
  const float min_std = lds[lay.misc()];
  float ob[brax::OBSB];  // what quad_observe reports: the raw [qpos, qvel]
#pragma unroll
  for (int j = 0; j < 3; j++) { ob[j] = e.pos[j]; ob[11 + j] = e.v[j]; ob[14 + j] = e.w[j]; }
#pragma unroll
  for (int j = 0; j < 4; j++) { ob[3 + j] = e.q[j]; ob[7 + j] = e.th[j]; ob[17 + j] = e.s[j]; }

  int32_t status = entry_status<KIND>(K, e);
  bool run = status == QUAD_PID_RUNNING;
  double ret = 0.0, err_sum = 0.0, err_sq = 0.0;
  int32_t steps = 0, err_count = 0;
  const uint32_t M = uint32_t(a.trace_envs);
  const bool traced = owner && uint32_t(i) < M;
  const uint64_t gid = p.gid_base + uint64_t(i);
  for (int t = 0; t < a.max_steps; t++) {
    if (!__any(run)) break;  // wave-uniform: the whole wave leaves together
    // ---- policy: the actor on the wave's tile, full wave (frozen lanes feed their columns too)
    float lg[brax::NLOG], ac[4];
    brax::forward<MB>(lds, packed, net, ob, lg);
    brax::env_action(lg, min_std, a.deterministic != 0, a.seed, gid, a.noise_step0 + uint32_t(t), ac);
    // ---- env step on a copy; a frozen env keeps its state
    EnvRegs<float> en = e;
    float obn[brax::OBSB], reward, motor[4];
    bool term, trunc;
    brax_step<float, KIND>(K, en, ac, obn, reward, term, trunc, motor);
    if (run) {
      const uint32_t row = uint32_t(t) * M + uint32_t(i);  // < 2^32 / 84: checked by quad_brax_episode
      if (traced) {
        if (a.trace_actions) sto(reinterpret_cast<float4*>(a.trace_actions), 16u * row, make_float4(ac[0], ac[1], ac[2], ac[3]));
        if (a.trace_obs) {
#pragma unroll
          for (int j = 0; j < brax::OBSB; j++) sto(a.trace_obs, 84u * row + 4u * j, ob[j]);
        }
      }
      e = en;
#pragma unroll
      for (int j = 0; j < brax::OBSB; j++) ob[j] = obn[j];
      {  // |pos - target| after the step with the step's target: float32 differences and norm, float64 sums
#pragma clang fp contract(off)
        const float d0 = e.pos[0] - e.target[0], d1 = e.pos[1] - e.target[1], d2 = e.pos[2] - e.target[2];
        const float er = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);  // libm's, correctly rounded (not fsqrt's v_sqrt_f32)
        if (q_abs(er) <= 3.4028235e38f) {
          err_sum += double(er);
          err_sq += double(er) * double(er);
          err_count += 1;
        }
        ret += double(reward);
      }
      steps += 1;
      if (traced) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
          if (a.trace_pos) sto(a.trace_pos, 12u * row + 4u * j, float(e.pos[j]));
          if (a.trace_target) sto(a.trace_target, 12u * row + 4u * j, float(e.target[j]));
        }
      }
      if (term || trunc) {
        status = term ? QUAD_PID_TERMINATED : QUAD_PID_TRUNCATED;
        run = false;
      }
    }
  }

  if (owner) {
    store_env(p, i, e, true);
    a.metrics.ret[i] = ret;
    a.metrics.steps[i] = steps;
    a.metrics.err_sum[i] = err_sum;
    a.metrics.err_sq_sum[i] = err_sq;
    a.metrics.err_count[i] = err_count;
    a.metrics.status[i] = status;
  }
}

}  // namespace

template <int BKIND, int MB>
hipError_t launch_brax_inst(const KConsts<float>* kc, const KParams& kp, const ActorNet& net, const float* packed,
                            const BraxEpisodeArgs& a, hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  const int bytes = brax::Layout{net.nb1, MB}.lds_bytes();  // <= 64 KB: no opt-in
  constexpr int KIND = BKIND == 1 ? QUAD_ENV_BRAX_TRAJ : QUAD_ENV_BRAX_HOVER;
  hipLaunchKernelGGL((k_brax_episode<KIND, MB>), dim3((kp.n + 63) / 64), dim3(128), bytes, s, kc, kp, packed, dn, a);
  return hipGetLastError();
}
template hipError_t launch_brax_inst<BA_KIND, BA_MB>(const KConsts<float>*, const KParams&, const ActorNet&, const float*,
                                                     const BraxEpisodeArgs&, hipStream_t);

}  // namespace quadenv

#else  // the C entry points' object

namespace {

int bfail(int code, const char* m) { return set_error(code, m); }

// ---- act / sample (actor_core.h act_tiles): logits and the NormalTanh action of a row; SAMPLE: the sampled action
// with its raw value and log-prob (brax_actor.h sample_action)
template <int MB, bool SAMPLE>
__global__ __launch_bounds__(actor::ACT_BLK) void k_brax_act(const float* __restrict__ packed, actor::Net net,
                                                             const float* __restrict__ obs, float* __restrict__ logits,
                                                             float* __restrict__ raw_out, float* __restrict__ logp_out,
                                                             float* __restrict__ actions_env, int32_t n,
                                                             int deterministic, uint64_t seed, uint64_t env_id_base,
                                                             uint32_t noise_step) {
  extern __shared__ float lds[];
  const brax::Layout lay{net.nb1, MB};
  actor::stage<actor::ACT_BLK>(lds, packed, lay.lds_floats());
  const float min_std = lds[lay.misc()];
  actor::act_tiles(n, [&](int row, bool ok, int h) {
    float ob[brax::OBSB], lg[brax::NLOG], ac[4], raw[4], logp = 0.f;
#pragma unroll
    for (int k = 0; k < brax::OBSB; k++) ob[k] = ok ? obs[size_t(row) * brax::OBSB + k] : 0.f;
    brax::forward<MB>(lds, packed, net, ob, lg);
    if constexpr (SAMPLE)
      brax::sample_action(lg, min_std, seed, env_id_base + uint64_t(row), noise_step, raw, logp, ac);
    else
      brax::env_action(lg, min_std, deterministic != 0, seed, env_id_base + uint64_t(row), noise_step, ac);
    if (!ok || h) return;  // one lane per row stores
    if (logits) {
#pragma unroll
      for (int k = 0; k < 2; k++)
        reinterpret_cast<float4*>(logits)[size_t(row) * 2 + k] = make_float4(lg[4 * k], lg[4 * k + 1], lg[4 * k + 2], lg[4 * k + 3]);
    }
    if constexpr (SAMPLE) {
      reinterpret_cast<float4*>(raw_out)[row] = make_float4(raw[0], raw[1], raw[2], raw[3]);
      logp_out[row] = logp;
    }
    reinterpret_cast<float4*>(actions_env)[row] = make_float4(ac[0], ac[1], ac[2], ac[3]);
  });
}

// the launch of both entry points (arguments checked by the caller)
template <bool SAMPLE>
hipError_t launch_brax_act(const ActorNet& net, const float* packed, const float* obs, float* logits, float* raw,
                           float* log_prob, float* actions_env, int32_t n, int deterministic, uint64_t seed,
                           uint64_t env_id_base, uint32_t noise_step, void* stream) {
  return with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const int bytes = brax::Layout{net.nb1, MB}.lds_bytes();
    hipLaunchKernelGGL((k_brax_act<MB, SAMPLE>), actor::act_grid(n), dim3(actor::ACT_BLK), bytes,
                       static_cast<hipStream_t>(stream), packed, actor::Net{net.nb1, net.actfn}, obs, logits, raw,
                       log_prob, actions_env, n, deterministic, seed, env_id_base, noise_step);
    return hipGetLastError();
  });
}

// QUAD_OK and *out, or QUAD_EINVAL with a message for an arch outside the family
int brax_net_of(const QuadBraxActorArch* a, ActorNet* out) { return actor::net_of(a, "brax actor arch", true, out); }

}  // namespace
}  // namespace quadenv

using namespace quadenv;

extern "C" {

int64_t quad_brax_actor_packed_floats(const QuadBraxActorArch* a) {
  ActorNet net;
  if (brax_net_of(a, &net)) return -1;
  return brax::Layout{net.nb1, net.mb}.floats();
}

int quad_brax_actor_pack(const QuadBraxActorArch* a, const QuadBraxActorParams* p, float* packed, void* stream) {
  ActorNet net;
  if (int rc = brax_net_of(a, &net)) return rc;
  if (!p || !packed) return bfail(QUAD_EINVAL, "quad_brax_actor_pack: params/packed is NULL");
  if (!p->w0 || !p->b0 || !p->w1 || !p->b1 || !p->w2 || !p->b2 || !p->mean || !p->std)
    return bfail(QUAD_EINVAL, "quad_brax_actor_pack: a parameter pointer is NULL");
  if (reinterpret_cast<uintptr_t>(packed) & 15u)
    return bfail(QUAD_EINVAL, "quad_brax_actor_pack: packed must be 16-byte aligned");
  const hipError_t e = actor::launch_pack<brax::Layout, false, brax::OBSB>(brax::Layout{net.nb1, net.mb}, *p, packed,
                                                                          static_cast<hipStream_t>(stream));
  return e == hipSuccess ? QUAD_OK : bfail(QUAD_EHIP, "k_brax_pack launch failed");
}

int quad_brax_actor_act(const QuadBraxActorArch* a, const float* packed, const float* obs, float* logits,
                        float* actions_env, int32_t n, int32_t deterministic, uint64_t seed, uint64_t env_id_base,
                        uint32_t noise_step, void* stream) {
  ActorNet net;
  if (int rc = brax_net_of(a, &net)) return rc;
  if (!packed || !obs || !actions_env) return bfail(QUAD_EINVAL, "quad_brax_actor_act: NULL argument");
  if (n <= 0) return bfail(QUAD_EINVAL, "quad_brax_actor_act: n must be > 0");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(actions_env) |
       reinterpret_cast<uintptr_t>(logits)) & 15u)
    return bfail(QUAD_EINVAL, "quad_brax_actor_act: packed, logits and actions_env must be 16-byte aligned");
  const hipError_t e = launch_brax_act<false>(net, packed, obs, logits, nullptr, nullptr, actions_env, n, deterministic,
                                             seed, env_id_base, noise_step, stream);
  return e == hipSuccess ? QUAD_OK : bfail(QUAD_EHIP, "k_brax_act launch failed");
}

int quad_brax_actor_sample(const QuadBraxActorArch* a, const float* packed, const float* obs, float* logits, float* raw,
                           float* log_prob, float* actions_env, int32_t n, uint64_t seed, uint64_t env_id_base,
                           uint32_t noise_step, void* stream) {
  ActorNet net;
  if (int rc = brax_net_of(a, &net)) return rc;
  if (!packed || !obs || !raw || !log_prob || !actions_env)
    return bfail(QUAD_EINVAL, "quad_brax_actor_sample: NULL argument");
  if (n <= 0) return bfail(QUAD_EINVAL, "quad_brax_actor_sample: n must be > 0");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(actions_env) |
       reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(logits)) & 15u)
    return bfail(QUAD_EINVAL, "quad_brax_actor_sample: packed, logits, raw and actions_env must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(log_prob) & 3u)
    return bfail(QUAD_EINVAL, "quad_brax_actor_sample: log_prob must be 4-byte aligned");
  const hipError_t e = launch_brax_act<true>(net, packed, obs, logits, raw, log_prob, actions_env, n, 0, seed,
                                            env_id_base, noise_step, stream);
  return e == hipSuccess ? QUAD_OK : bfail(QUAD_EHIP, "k_brax_act launch failed");
}

// ---- whole episodes on the brax kinds (k_brax_episode)
int quad_brax_episode(QuadHandle* h, const QuadBraxActorArch* arch, const float* packed, const QuadBraxRun* r,
                      void* stream) {
  const auto bad = [](const char* m) { return fail(QUAD_EINVAL, std::string("quad_brax_episode: ") + m); };
  ActorNet net;
  if (int rc = brax_net_of(arch, &net)) return rc;
  if (!h || !packed || !r) return bad("handle/packed/run is NULL");
  if (h->cfg.env_kind != QUAD_ENV_BRAX_HOVER && h->cfg.env_kind != QUAD_ENV_BRAX_TRAJ)
    return bad("env_kind must be BRAX_HOVER or BRAX_TRAJ");
  if (r->max_steps < 1) return bad("max_steps must be >= 1");
  const QuadBraxMetrics& m = r->metrics;
  if (!m.ret || !m.steps || !m.err_sum || !m.err_sq_sum || !m.err_count || !m.status)
    return bad("every metrics array is required");
  if (r->trace_envs < 0 || r->trace_envs > h->n) return bad("trace_envs must be in [0, N]");
  if (reinterpret_cast<uintptr_t>(packed) & 15u) return bad("packed must be 16-byte aligned");
  const bool any_trace = r->trace_actions || r->trace_obs || r->trace_pos || r->trace_target;
  if (any_trace && r->trace_envs > 0) {
    if (int64_t(r->max_steps) * r->trace_envs * 84 > int64_t(UINT32_MAX))
      return bad("max_steps * trace_envs too large (trace rows use 32-bit byte offsets)");
    if (reinterpret_cast<uintptr_t>(r->trace_actions) & 15u) return bad("the action trace must be 16-byte aligned");
  }
  const BraxEpisodeArgs a{r->max_steps, any_trace ? r->trace_envs : 0, r->deterministic, r->noise_step0, r->seed,
                          r->metrics, r->trace_actions, r->trace_obs, r->trace_pos, r->trace_target};
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    return h->cfg.env_kind == QUAD_ENV_BRAX_TRAJ ? launch_brax_inst<1, MB>(h->kdev, h->kp, net, packed, a, s)
                                                 : launch_brax_inst<0, MB>(h->kdev, h->kp, net, packed, a, s);
  }));
  return QUAD_OK;
}

// ---- the Brax learner's unrolls on the brax kinds (k_brax_unroll, brax_unroll.hip)
int quad_brax_unroll(QuadHandle* h, const QuadBraxActorArch* arch, const float* packed, const QuadBraxUnroll* u,
                     void* stream) {
  const auto bad = [](const char* m) { return fail(QUAD_EINVAL, std::string("quad_brax_unroll: ") + m); };
  ActorNet net;
  if (int rc = brax_net_of(arch, &net)) return rc;
  if (!h || !packed || !u) return bad("handle/packed/unroll is NULL");
  if (h->cfg.env_kind != QUAD_ENV_BRAX_HOVER && h->cfg.env_kind != QUAD_ENV_BRAX_TRAJ)
    return bad("env_kind must be BRAX_HOVER or BRAX_TRAJ");
  if (!h->cfg.auto_reset) return bad("the handle must have auto_reset = 1");
  if (u->steps < 1 || u->unroll_length < 1) return bad("steps and unroll_length must be >= 1");
  if (u->steps % u->unroll_length) return bad("steps must be a multiple of unroll_length");
  if (!u->obs || !u->raw || !u->log_prob || !u->reward || !u->discount || !u->truncation || !u->next_obs ||
      !u->ep_ret || !u->stats)
    return bad("every buffer is required");
  const auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  if ((at(packed) | at(u->raw)) & 15u) return bad("packed and raw must be 16-byte aligned");
  if ((at(u->obs) | at(u->log_prob) | at(u->reward) | at(u->discount) | at(u->truncation) | at(u->next_obs) |
       at(u->ep_ret)) & 3u)
    return bad("the float buffers must be 4-byte aligned");
  if (at(u->stats) & 7u) return bad("stats must be 8-byte aligned");
  if (int64_t(u->steps) * h->n * 84 > int64_t(UINT32_MAX))
    return bad("steps * N too large (rows use 32-bit byte offsets)");
  const BraxUnrollArgs a{u->obs, u->raw, u->log_prob, u->reward, u->discount, u->truncation, u->next_obs, u->ep_ret,
                         u->stats, u->steps, u->unroll_length, u->noise_step0, u->seed};
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    return h->cfg.env_kind == QUAD_ENV_BRAX_TRAJ ? launch_brax_unroll_inst<1, MB>(h->kdev, h->kp, net, packed, a, s)
                                                 : launch_brax_unroll_inst<0, MB>(h->kdev, h->kp, net, packed, a, s);
  }));
  return QUAD_OK;
}

}  // extern "C"
#endif
