// brax_unroll.hip -- the Brax learner's unrolls in one launch (quad_brax_unroll): `steps` whole steps of
// ppo/brax_ppo.py BraxPPO._unrolls on a brax env kind with auto-reset.
//
// Kernel
//   k_brax_unroll<KIND, MB>   the episode kernel's block shape (brax_actor.hip k_brax_episode): 64-env blocks of two
//                             one-tile waves, every env's state in registers for all steps, the packed image staged in
//                             LDS once. Per step: observation row -> forward -> NormalTanh sample and log-prob ->
//                             brax_step on tanh(raw) -> reward / discount / truncation rows -> Monitor accounting ->
//                             k_step_brax's auto-reset; after every unroll_length steps the next_obs row.
//
// The two rules of brax_actor.hip keep the launch bit-identical to quad_brax_actor_sample + quad_step per step: the
// forward, the draw and the log-prob are brax_actor.h's one definition, executed by the full wave outside every
// per-lane branch; and this file is built with quadenv.o's floating-point flags (-ffp-contract=on, no SLP
// vectorizer), so brax_step and the reset have k_step_brax's bits.
//
// Compiled once per (BU_KIND, BU_MB): BU_KIND = 0 brax hover / 1 brax trajectory, BU_MB = H2 / 32 = 2 / 4 / 8. The
// launch dispatch over the six objects is quad_brax_unroll's (brax_actor.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "brax_actor.h"
#include "env_tiles.h"
#include "quad_physics.h"

#if !defined(BU_KIND) || !defined(BU_MB)
#error "brax_unroll.hip is built per (BU_KIND, BU_MB): see the Makefile"
#endif

namespace quadenv {

namespace {

template <int KIND, int MB>
__global__ __launch_bounds__(128) void k_brax_unroll(const KConsts<float>* __restrict__ kc, KParams p,
                                                     const float* __restrict__ packed, actor::Net net,
                                                     BraxUnrollArgs a) {
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
  // the running episode is counter - 1: AutoResetWrapper returns to its first state and leaves the counter alone
  const uint32_t ep = Tiles(p).ldu(F_EP, env_off(uint32_t(i)));
  settle(ep);
  float ret = a.ep_ret[i];
  actor::stage<128>(lds, packed, lay.lds_floats());
  const float min_std = lds[lay.misc()];
  float ob[brax::OBSB];  // what quad_observe reports: the raw [qpos, qvel]
#pragma unroll
  for (int j = 0; j < 3; j++) { ob[j] = e.pos[j]; ob[11 + j] = e.v[j]; ob[14 + j] = e.w[j]; }
#pragma unroll
  for (int j = 0; j < 4; j++) { ob[3 + j] = e.q[j]; ob[7 + j] = e.th[j]; ob[17 + j] = e.s[j]; }

  const uint64_t gid = p.gid_base + uint64_t(i);
  const uint32_t n = uint32_t(p.n);
  double st_ret = 0.0, st_cnt = 0.0;  // owner lanes only
  int32_t left = a.unroll_length;     // steps to the next next_obs row
  uint32_t unroll = 0;
  for (int t = 0; t < a.steps; t++) {
    const uint32_t row = uint32_t(t) * n + uint32_t(i);  // < 2^32 / 84: checked by quad_brax_unroll
    if (owner) {
#pragma unroll
      for (int j = 0; j < brax::OBSB; j++) sto(a.obs, 84u * row + 4u * j, ob[j]);
    }
    // ---- policy: the actor on the wave's tile, full wave
    float lg[brax::NLOG], raw[4], ac[4], logp;
    brax::forward<MB>(lds, packed, net, ob, lg);
    brax::sample_action(lg, min_std, a.seed, gid, a.noise_step0 + uint32_t(t), raw, logp, ac);
    // ---- env step
    float reward, motor[4];
    bool term, trunc;
    brax_step<float, KIND>(K, e, ac, ob, reward, term, trunc, motor);
    const bool done = term || trunc;
    ret = __fadd_rn(ret, reward);
    if (owner) {
      sto(reinterpret_cast<float4*>(a.raw), 16u * row, make_float4(raw[0], raw[1], raw[2], raw[3]));
      sto(a.log_prob, 4u * row, logp);
      sto(a.reward, 4u * row, reward);
      sto(a.discount, 4u * row, done ? 0.f : 1.f);
      sto(a.truncation, 4u * row, (trunc && !term) ? 1.f : 0.f);  // EpisodeWrapper info['truncation']
      if (done) { st_ret += double(ret); st_cnt += 1.0; }
    }
    if (done) {  // k_step_brax's auto-reset: the first state of the episode, from its draw
      ret = 0.f;
      float u21[21];
      brax_reset_draw(K.bx_noise, p.seed, gid, ep - 1u, u21);
      brax_reset_from<float, KIND>(K, e, u21, ob, true);
    }
    if (--left == 0) {
      left = a.unroll_length;
      if (owner) {
        const uint32_t nrow = unroll * n + uint32_t(i);
#pragma unroll
        for (int j = 0; j < brax::OBSB; j++) sto(a.next_obs, 84u * nrow + 4u * j, ob[j]);
      }
      unroll += 1u;
    }
  }

  if (owner) {
    store_env(p, i, e, true);
    a.ep_ret[i] = ret;
  }
  // Monitor statistics: block sum into this block's slot (uncontended double atomics), as k_rollout's
  __shared__ double red[2][2];
  {
    double v0 = owner ? st_ret : 0.0, v1 = owner ? st_cnt : 0.0;
    for (int off = 32; off > 0; off >>= 1) { v0 += __shfl_down(v0, off); v1 += __shfl_down(v1, off); }
    if ((threadIdx.x & 63) == 0) { red[0][w] = v0; red[1][w] = v1; }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double s = red[threadIdx.x][0] + red[threadIdx.x][1];
    if (s != 0.0) atomicAdd(&a.stats[(blockIdx.x % QUAD_POLICY_STAT_SLOTS) * 2 + threadIdx.x], s);
  }
}

}  // namespace

template <int BKIND, int MB>
hipError_t launch_brax_unroll_inst(const KConsts<float>* kc, const KParams& kp, const ActorNet& net, const float* packed,
                                   const BraxUnrollArgs& a, hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  const int bytes = brax::Layout{net.nb1, MB}.lds_bytes();  // <= 64 KB: no opt-in
  constexpr int KIND = BKIND == 1 ? QUAD_ENV_BRAX_TRAJ : QUAD_ENV_BRAX_HOVER;
  hipLaunchKernelGGL((k_brax_unroll<KIND, MB>), dim3((kp.n + 63) / 64), dim3(128), bytes, s, kc, kp, packed, dn, a);
  return hipGetLastError();
}
template hipError_t launch_brax_unroll_inst<BU_KIND, BU_MB>(const KConsts<float>*, const KParams&, const ActorNet&,
                                                            const float*, const BraxUnrollArgs&, hipStream_t);

}  // namespace quadenv
