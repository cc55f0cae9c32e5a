// actor_rollout.hip -- the PPO rollout of the general actor's family (actor_arch.h: 12 -> H1 -> H2 -> 4 / 1, ReLU or
// tanh, policy and value net of the same widths): policy.hip's per-step kernel and rollout.hip's one-launch kernel
// with actor_core.h's forward in the 128 net's place (quad_actor_critic_* / quad_actor_rollout, include/quadenv.h).
//
// Packed image (floats; A = arch::Layout{H1 / 32, H2 / 32}.floats() = quad_actor_packed_floats):
//   [0, A)       the policy net's image, quad_actor_pack's to the bit (the same pack kernel on the same parameters)
//   [A, 2A)      the value net's image in the same layout: a head of four outputs whose rows 1..3 and biases 1..3
//                are zero, so output 0 of the forward is V
//   [2A, 2A + 4) log_std
// quad_actor_critic_pack is three stream-ordered launches: k_ac_head writes the value head zero-padded to [4, H2] +
// [4] into the first floats of the image (the policy half, still unwritten) and log_std into its place; the pack
// kernel writes the value half from there; the pack kernel writes the policy half over the padded head.
//
// Kernels
//   k_ac_head                   the padded value head and log_std (above)
//   k_ac_act<MB>                k_policy_act's contract on k_actor_act's tile loop: per 32-row tile the epilogue of
//                               step t - 1 when the cursor marks it pending, the forward of both nets over one split
//                               of the observation fragment, the Gaussian sample, its log-prob and the clip
//   k_ac_post<MB>               k_rollout_post's contract: the pending epilogue alone (the value image only)
//   k_ac_rollout<KIND, CTBR, MB>  rollout_body's NT = 1 structure on the episode kernels' block shape: 64-env blocks
//                               of two one-tile waves, env state and observation in registers for all steps, both
//                               images' LDS parts staged once, the W2 pieces streamed from L2; a block with at most
//                               32 envs runs its two nets on its two waves (split blocks, see the kernel)
//   k_ac_rollout_deployed<KIND, CTBR, MB>  k_ac_rollout acting on quad_deploy.h's observation: the velocity estimator
//                               in registers beside the env, updated after every step and emptied by a reset
//   k_pop_ac_head, k_pop_ac_pack, k_pop_ac_value<MB>, k_pop_ac_rollout<KIND, CTBR, MB>
//                               the population forms (population.h): the bodies of k_ac_head, the pack
//                               kernel, k_ac_act and k_ac_rollout behind one more grid dimension, the member's
//                               arguments read from a device table
//   k_pop_ac_rollout_deployed<KIND, CTBR, MB>  k_ac_rollout_deployed's population form: the member's
//                               estimator arguments from a second table, pop::EstEntry
//
// The sample, the log-prob, the reward row and the forward of either net are one definition each, used by both
// forms, and this file is built with the episode objects' floating-point flags (-ffp-contract=on, no SLP
// vectorizer), so env_step and the reset have k_step_h's bits: the one-launch form is bit-identical to k_ac_act +
// quad_step per step + k_ac_post.
//
// Compiled once without AR_KIND (the entry points, k_ac_head / k_ac_act / k_ac_post, the launch dispatch) and once
// per (AR_KIND, AR_MB): AR_KIND = 0 hover / 1 trajectory, AR_MB = H2 / 32 = 2 / 4 / 8 -- six objects of two
// kernels each (CTBR or not) that build in parallel, and six more with AR_DEPLOYED: k_ac_rollout_deployed and
// k_pop_ac_rollout_deployed, the body in its deployed-observation mode (quad_actor_rollout_deployed).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/quadenv.h"
#include "actor_arch.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "handle.h"
#include "policy_episode.h"
#include "population.h"
#include "quad_deploy.h"
#include "quad_physics.h"
#include "rollout.h"

namespace quadenv {

// one (kind, MB) object's instantiations, defined and explicitly instantiated in that object
template <int AKIND, int MB>
hipError_t launch_actor_rollout_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                                     const float* packed, const RollArgs& a, hipStream_t s);
template <int AKIND, int MB>
hipError_t launch_pop_actor_rollout_inst(const KConsts<float>* kc, const pop::RollEntry* tab, const int32_t* active,
                                         int count, int n, bool ctbr, const ActorNet& net, uint32_t t0, int32_t steps,
                                         hipStream_t s);
// one (kind, MB) deployed object's instantiations (AR_DEPLOYED)
template <int AKIND, int MB>
hipError_t launch_actor_rollout_deployed_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                                              const float* packed, const RollArgs& a, const EstArgs& est, double est_dt,
                                              hipStream_t s);
template <int AKIND, int MB>
hipError_t launch_pop_actor_rollout_deployed_inst(const KConsts<float>* kc, const pop::RollEntry* tab,
                                                  const pop::EstEntry* etab, const int32_t* active, int count, int n,
                                                  bool ctbr, const ActorNet& net, uint32_t t0, int32_t steps,
                                                  hipStream_t s);

namespace {

// The nets k0 .. k1 - 1 of one tile (0: the policy net, 1: the value net) over one split of the observation fragment:
// the four means, and V = the value image's output 0. One forward in the code, run once per net; k0 and k1 are
// wave-uniform ((0, 2) everywhere but in k_ac_rollout's split blocks). La / Lc: the staged images; packed: the global
// image (the W2 pieces are read from it)
template <int MB>
__device__ __forceinline__ void forward_nets(const float* __restrict__ La, const float* __restrict__ Lc,
                                             const float* packed, const actor::Net& net, const float (&xq)[8], int k0,
                                             int k1, float (&mean)[ACT], float& val) {
  const arch::Layout lay{net.nb1, MB};
  const P3 xp = split8(xq);
#pragma unroll 1
  for (int k = k0; k < k1; k++) {
    gbf16x8* w = actor::lane_pieces(packed + (k ? lay.floats() : 0) + lay.w2p());
    float o[ACT];
    actor::forward<MB, 2>(k ? Lc : La, lay, net.actfn, xp, xp, w, w, o);
    if (k) {
      val = o[0];
    } else {
#pragma unroll
      for (int q = 0; q < ACT; q++) mean[q] = o[q];
    }
  }
}

template <int MB>
__device__ __forceinline__ void forward_ac(const float* __restrict__ La, const float* __restrict__ Lc,
                                           const float* packed, const actor::Net& net, const float (&xq)[8],
                                           float (&mean)[ACT], float& val) {
  forward_nets<MB>(La, Lc, packed, net, xq, 0, 2, mean, val);
}

// the value net alone (the TimeLimit bootstrap's V(terminal_obs))
template <int MB>
__device__ __forceinline__ float forward_v(const float* __restrict__ Lc, const float* packed, const actor::Net& net,
                                           const float (&xq)[8]) {
  float mean[ACT], val = 0.f;
  forward_nets<MB>(Lc, Lc, packed, net, xq, 1, 2, mean, val);
  return val;
}

// the Gaussian action of one env (SB3 policy.forward: a = mean + std z, z from Philox(seed; env id, t, 0x200)), its
// log-prob recomputed from the stored action as PPO.train does, and the clipped action the env receives
__device__ __forceinline__ void sample_action(bool deterministic, uint64_t seed, uint64_t gid, uint32_t t,
                                              const float (&mean)[ACT], const float (&sd)[ACT],
                                              const float (&lstd)[ACT], float (&act)[ACT], float (&ac)[ACT],
                                              float& lp) {
  float z[ACT] = {0.f, 0.f, 0.f, 0.f};
  if (!deterministic) gauss4(seed, gid, t, z);
  lp = 0.f;
#pragma unroll
  for (int k = 0; k < ACT; k++) {
    act[k] = mean[k] + sd[k] * z[k];
    const float zz = (act[k] - mean[k]) / sd[k];  // policy.log_prob on the stored action
    lp += -0.5f * zz * zz - lstd[k] - 0.91893853320467274f;  // 0.5 log(2 pi)
    ac[k] = fminf(fmaxf(act[k], -1.f), 1.f);
  }
}

// the reward row: r + gamma V(terminal_obs) on a time-limit truncation
__device__ __forceinline__ float reward_row(bool timeout, float reward, float gamma, float tv) {
  return timeout ? reward + gamma * tv : reward;
}

}  // namespace

#if defined(AR_KIND)
namespace {

// The reset draws of the wave's resetting envs, compacted across the wave (rollout.hip's reset_words_shfl with
// lanes l and l + 32 carrying the same env): one Philox pass of (env, block) items for up to 16 resetting envs,
// the words travelling by lane shuffles. `publish`: this lane lists its env (one lane per env); `apply`: this lane
// takes the words of the env listed under its rank.
__device__ __forceinline__ void reset_words_shfl(const KParams& p, uint32_t (&renv)[64], uint32_t (&rep)[64], uint32_t i,
                                                 uint32_t ep, bool publish, bool apply, float u16[16]) {
  const uint64_t m = __ballot(publish);
  if (m == 0) return;
  const int lane = __lane_id();
  const int nres = __popcll(m);
  const int rank = __popcll(m & ((1ull << (lane & 31)) - 1ull));
  if (publish) { renv[rank] = i; rep[rank] = ep; }
  __builtin_amdgcn_wave_barrier();
  const int passes = (nres * 4 + 63) >> 6;
  for (int t = 0; t < passes; t++) {
    const int item = t * 64 + lane, rr = item >> 2;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    if (rr < nres) reset_block(p.seed, p.gid_base + uint64_t(renv[rr]), rep[rr], uint32_t(item & 3), c);
    float cu[4];
#pragma unroll
    for (int k = 0; k < 4; k++) cu[k] = u01(c[k]);
    const bool mine = apply && (rank >> 4) == t;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int src = (rank * 4 + b) & 63;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float v = __shfl(cu[k], src);
        if (mine) u16[4 * b + k] = v;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// (the time-major rows can lie past 4 GiB)
__device__ __forceinline__ void store_row(float* __restrict__ base, size_t row, const float v[12]) {
  float4* b4 = reinterpret_cast<float4*>(base + row * 12);
  b4[0] = make_float4(v[0], v[1], v[2], v[3]);
  b4[1] = make_float4(v[4], v[5], v[6], v[7]);
  b4[2] = make_float4(v[8], v[9], v[10], v[11]);
}

// k_ac_rollout's body, shared with the population form below (p.kc is the launch's noalias constant block).
// MODE = QUAD_OBS_DEPLOYED (k_ac_rollout_deployed; est / est_dt are read in that mode only): the row in hand is the
// deployed one. Every lane keeps its env's estimator (quad_deploy.h: eight float64 words, and alpha) in registers for
// all steps and updates it after the env step, on the step's state12 at the new step count; the row D it builds
// feeds the bootstrap and is the next row in hand. A reset empties the estimator and updates it once with the reset
// state. In a split block both waves run the same update on the same values, so V(D) on the value wave is V of the
// row the policy wave stores; the policy wave stores the estimators.
template <int KIND, bool CTBR, int MB, int MODE = QUAD_OBS_ENV>
__device__ __forceinline__ void ac_rollout_body(const KConsts<float>& K, KParams p, const float* __restrict__ packed,
                                                actor::Net net, RollArgs a, EstArgs est = EstArgs{},
                                                double est_dt = 0.0) {
  constexpr bool DEP = MODE == QUAD_OBS_DEPLOYED;
  extern __shared__ float lds[];
  __shared__ uint32_t renv[2][64], rep[2][64];
  __shared__ float4 xmean[2][32];
  const arch::Layout lay{net.nb1, MB};
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // a scalar: it selects the wave's nets
  const bool h = (threadIdx.x & 32) != 0;
  // A block whose second wave would hold no env (the last block of a ragged n; the only block at the reference's 16
  // envs) is SPLIT: both waves carry the first tile's envs and step them alike (the same code on the same values:
  // the same bits), wave 0 runs the policy net, wave 1 the value net, beside each other instead of one after the
  // other. Wave 0 hands the means over through LDS (one barrier per step, two buffers); wave 1 stores the value and
  // reward rows, wave 0 everything else. Block-uniform, so the barrier is taken by both waves or by neither.
  const bool split = blockIdx.x * 64 + 32 >= p.n;
  const bool vwave = split && w == 1;
  const int i_raw = blockIdx.x * 64 + (split ? 0 : w * 32) + int(threadIdx.x & 31);
  const bool ok = i_raw < p.n;
  const bool owner = ok && !h;  // lanes l and l + 32 carry env l & 31 (the same bits); the lower half stores
  const bool own_pi = owner && !vwave, own_v = owner && (!split || vwave);  // who stores which rows
  const int k0 = vwave ? 1 : 0, k1 = split && !vwave ? 1 : 2;               // this wave's nets
  // lanes past the last env shadow it (in-range loads, MFMA columns of their own) and store nothing
  const int i = ok ? i_raw : p.n - 1;
  const size_t n = size_t(p.n);

  // ---- per-env state into registers (issued before the weight staging so both are in flight)
  EnvRegs<float> e;
  load_env(p, i, e, CTBR);
  const Tiles S(p);
  const uint32_t vo = env_off(uint32_t(i));
  uint32_t ep = S.ldu(F_EP, vo);
  float ob[12];
  {
    const float4* r4 = reinterpret_cast<const float4*>(a.last_obs + size_t(i) * 12);
    const float4 x0 = r4[0], x1 = r4[1], x2 = r4[2];
    ob[0] = x0.x; ob[1] = x0.y; ob[2] = x0.z; ob[3] = x0.w;
    ob[4] = x1.x; ob[5] = x1.y; ob[6] = x1.z; ob[7] = x1.w;
    ob[8] = x2.x; ob[9] = x2.y; ob[10] = x2.z; ob[11] = x2.w;
  }
  float ls = a.last_start[i], ret = a.ep_ret[i], len = a.ep_len[i];
  double ve[EST_NSTATE] = {}, alpha = 0.0;
  if constexpr (DEP) {
    alpha = est.alpha ? est.alpha[i] : est.alpha_all;
#pragma unroll
    for (int j = 0; j < EST_NSTATE; j++) ve[j] = est.state[size_t(j) * n + size_t(i)];
  }
  // both images' LDS parts, once per launch: the policy net's at 0, the value net's behind it
  float* Lc = lds + lay.lds_floats();
  {
    const int nv = lay.lds_floats() / 4;
    const float4* sa = reinterpret_cast<const float4*>(packed);
    const float4* sc = reinterpret_cast<const float4*>(packed + lay.floats());
    float4* da = reinterpret_cast<float4*>(lds);
    float4* dc = reinterpret_cast<float4*>(Lc);
    for (int k = threadIdx.x; k < nv; k += 128) { da[k] = sa[k]; dc[k] = sc[k]; }
    __syncthreads();
  }
  const float* log_std = packed + 2 * lay.floats();
  float lstd[ACT], sd[ACT];
#pragma unroll
  for (int k = 0; k < ACT; k++) { lstd[k] = log_std[k]; sd[k] = expf(lstd[k]); }
  double st[3] = {0.0, 0.0, 0.0};
  const uint64_t gid = p.gid_base + uint64_t(i);

  for (int s = 0; s < a.steps; s++) {
    const uint32_t t = a.t0 + uint32_t(s);
    const size_t row = size_t(t % a.rows) * n + size_t(i);
    // ---- policy: both nets on the wave's tile, then this lane's env
    float xb[1][8], mean[ACT] = {0.f, 0.f, 0.f, 0.f}, val = 0.f;
    fragments<1>(ob, xb);
    forward_nets<MB>(lds, Lc, packed, net, xb[0], k0, k1, mean, val);
    if (split) {
      if (own_pi) xmean[s & 1][threadIdx.x & 31] = make_float4(mean[0], mean[1], mean[2], mean[3]);
      __syncthreads();
      if (vwave) {
        const float4 m = xmean[s & 1][threadIdx.x & 31];
        mean[0] = m.x; mean[1] = m.y; mean[2] = m.z; mean[3] = m.w;
      }
    }
    float act[ACT], ac[ACT], lp;
    sample_action(a.deterministic != 0, a.seed, gid, t, mean, sd, lstd, act, ac, lp);
    if (own_pi) {
      store_row(a.obs_copy, row, ob);
      reinterpret_cast<float4*>(a.actions)[row] = make_float4(act[0], act[1], act[2], act[3]);
      a.log_prob[row] = lp;
      a.starts[row] = ls;
    }
    if (own_v) a.value[row] = val;
    // ---- env step (HoverEnv.step / TrajectoryFollowEnv.step, RateControlWrapper.action)
    StepRes r;
    env_step<float, CTBR>(K, e, ac, r);
    const bool done = r.term || r.trunc;
    if constexpr (DEP) {  // row D: the estimator's sample of this step, the step's own target (before any reset)
      double vel[3];
      vel_est_update(alpha, est.max_dt, r.state12, double(e.step) * est_dt, ve, vel);
      deploy_obs(K.obs_lo, K.obs_span, K.obs_rspan, r.state12, e.target, vel, r.obs);
    }
    // ---- TimeLimit bootstrap: r += gamma V(terminal_obs) (the value net only if the wave holds one)
    const bool timeout = ok && r.trunc && !r.term;
    float tv = 0.f;
    if (__any(timeout) && k1 == 2) {  // (a split block's policy wave stores no reward row)
      float xt[1][8];
      fragments<1>(r.obs, xt);
      tv = forward_v<MB>(Lc, packed, net, xt[0]);
    }
    // ---- reward row, Monitor statistics, episode_starts of the next step
    const float rret = ret + r.reward, rlen = len + 1.f;
    if (own_v) a.rewards[row] = reward_row(timeout, r.reward, a.gamma, tv);
    if (own_pi && done) { st[0] += double(rret); st[1] += double(rlen); st[2] += 1.0; }  // one lane per env
    ret = done ? 0.f : rret;
    len = done ? 0.f : rlen;
    ls = done ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < 12; j++) ob[j] = r.obs[j];
    // ---- SB3 auto-reset: the next step starts from the reset observation
    const bool rs = ok && done;
    float u16[16];
    reset_words_shfl(p, renv[w], rep[w], uint32_t(i), ep, owner && done, rs, u16);
    if (rs) {
      float init12[12], tgt[3], s12[12];
      reset_affine_u(K.init_lo, K.init_span, K.tgt_lo, K.tgt_span, u16, init12, tgt);
      env_reset_from<float, KIND>(K, e, init12, tgt, ob, s12);
      ep += 1u;
      if constexpr (DEP) {  // a new VelocityEstimator, its first sample the reset state: velocity 0
        // the state as quad_observe reports it (the attitude read back from the quaternion, as the node reads the
        // mocap's and as the episode kernels' first row has it), not the drawn Euler angles
        observe(K, e, ob, s12);
        double vel[3];
#pragma unroll
        for (int j = 0; j < EST_NSTATE; j++) ve[j] = 0.0;
        vel_est_update(alpha, est.max_dt, s12, double(e.step) * est_dt, ve, vel);
        deploy_obs(K.obs_lo, K.obs_span, K.obs_rspan, s12, e.target, vel, ob);
      }
    }
  }

  // ---- carry the rollout to the next call
  if (own_pi) {
    store_env(p, i, e, CTBR);
    S.stu(F_EP, vo, ep);
    store_row(a.last_obs, size_t(i), ob);
    a.last_start[i] = ls;
    a.ep_ret[i] = ret;
    a.ep_len[i] = len;
    if constexpr (DEP) {
#pragma unroll
      for (int j = 0; j < EST_NSTATE; j++) est.state[size_t(j) * n + size_t(i)] = ve[j];
    }
  }
  // Monitor statistics: block sum into this block's slot (uncontended double atomics), as k_rollout's
  __shared__ double red[3][2];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double v = st[j];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) red[j][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double s = red[threadIdx.x][0] + red[threadIdx.x][1];
    if (s != 0.0) atomicAdd(&a.stats[(blockIdx.x % QUAD_POLICY_STAT_SLOTS) * 3 + threadIdx.x], s);
  }
}

#if defined(AR_DEPLOYED)  // the deployed objects: k_ac_rollout's body in QUAD_OBS_DEPLOYED mode, and its launch
template <int KIND, bool CTBR, int MB>
__global__ __launch_bounds__(128) void k_ac_rollout_deployed(const KConsts<float>* __restrict__ kc, KParams p,
                                                             const float* __restrict__ packed, actor::Net net,
                                                             RollArgs a, EstArgs est, double est_dt) {
  p.kc = kc;  // (k_ac_rollout's note)
  ac_rollout_body<KIND, CTBR, MB, QUAD_OBS_DEPLOYED>(*kc, p, packed, net, a, est, est_dt);
}

// The population form (population.h): block (b, k) is block b of member active[k]'s
// quad_actor_rollout_deployed. The member's rollout entry is k_pop_ac_rollout's, read the same way; its estimator
// arguments and est_dt come from a table of their own (pop::EstEntry, indexed by member), read through
// pop::const_entry too: the body reads them once, before its step loop, into the registers the single kernel's
// arguments reach it in.
template <int KIND, bool CTBR, int MB>
__global__ __launch_bounds__(128) void k_pop_ac_rollout_deployed(const KConsts<float>* __restrict__ kc,
                                                                 const pop::RollEntry* __restrict__ tab,
                                                                 const pop::EstEntry* __restrict__ etab,
                                                                 const int32_t* __restrict__ active, actor::Net net,
                                                                 uint32_t t0, int32_t steps) {
#if defined(__HIP_DEVICE_COMPILE__)  // (pop::const_entry, population.h)
  const int32_t m = active[blockIdx.y];
  const auto& en = pop::const_entry(tab, m);
  const auto& ee = pop::const_entry(etab, m);
  KParams p = en.kp;
  p.kc = kc;
  RollArgs a = en.a;
  a.t0 = t0;
  a.steps = steps;
  const float* __restrict__ packed = en.packed;
  const EstArgs est = ee.est;
  ac_rollout_body<KIND, CTBR, MB, QUAD_OBS_DEPLOYED>(*kc, p, packed, net, a, est, ee.est_dt);
#endif
}

}  // namespace

template <int AKIND, int MB>
hipError_t launch_pop_actor_rollout_deployed_inst(const KConsts<float>* kc, const pop::RollEntry* tab,
                                                  const pop::EstEntry* etab, const int32_t* active, int count, int n,
                                                  bool ctbr, const ActorNet& net, uint32_t t0, int32_t steps,
                                                  hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  constexpr int MAX_BYTES = 2 * arch::Layout{actor::MAX_H1 / 32, MB}.lds_bytes();  // (launch_actor_rollout_inst's rule)
  const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
  constexpr int KIND = AKIND == 1 ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
  const dim3 grid((n + 63) / 64, count), block(128);
  return with_bool(ctbr, [&](auto cb) {
    constexpr bool CB = decltype(cb)::value;
    if (const hipError_t e = lds_opt_in<&k_pop_ac_rollout_deployed<KIND, CB, MB>>(MAX_BYTES)) return e;
    return launch_lds<&k_pop_ac_rollout_deployed<KIND, CB, MB>>(grid, block, bytes, s, kc, tab, etab, active, dn, t0,
                                                                 steps);
  });
}
template hipError_t launch_pop_actor_rollout_deployed_inst<AR_KIND, AR_MB>(const KConsts<float>*, const pop::RollEntry*,
                                                                           const pop::EstEntry*, const int32_t*, int,
                                                                           int, bool, const ActorNet&, uint32_t,
                                                                           int32_t, hipStream_t);

template <int AKIND, int MB>
hipError_t launch_actor_rollout_deployed_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                                              const float* packed, const RollArgs& a, const EstArgs& est, double est_dt,
                                              hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  constexpr int MAX_BYTES = 2 * arch::Layout{actor::MAX_H1 / 32, MB}.lds_bytes();  // (launch_actor_rollout_inst's rule)
  const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
  constexpr int KIND = AKIND == 1 ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
  const dim3 grid((kp.n + 63) / 64), block(128);
  return with_bool(ctbr, [&](auto cb) {
    constexpr bool CB = decltype(cb)::value;
    if (const hipError_t e = lds_opt_in<&k_ac_rollout_deployed<KIND, CB, MB>>(MAX_BYTES)) return e;
    return launch_lds<&k_ac_rollout_deployed<KIND, CB, MB>>(grid, block, bytes, s, kc, kp, packed, dn, a, est, est_dt);
  });
}
template hipError_t launch_actor_rollout_deployed_inst<AR_KIND, AR_MB>(const KConsts<float>*, const KParams&, bool,
                                                                       const ActorNet&, const float*, const RollArgs&,
                                                                       const EstArgs&, double, hipStream_t);

}  // namespace quadenv

#else  // the env-observation objects
template <int KIND, bool CTBR, int MB>
__global__ __launch_bounds__(128) void k_ac_rollout(const KConsts<float>* __restrict__ kc, KParams p,
                                                    const float* __restrict__ packed, actor::Net net, RollArgs a) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  ac_rollout_body<KIND, CTBR, MB>(*kc, p, packed, net, a);
}

// The population form (population.h): block (b, k) is block b of member active[k]'s rollout. As in k_pop_rollout the
// member's entry is read through pop::const_entry, t0 / steps come with the launch, and the constant block -- the
// same for every member, like the arch -- stays the noalias kernel argument.
template <int KIND, bool CTBR, int MB>
__global__ __launch_bounds__(128) void k_pop_ac_rollout(const KConsts<float>* __restrict__ kc,
                                                        const pop::RollEntry* __restrict__ tab,
                                                        const int32_t* __restrict__ active, actor::Net net, uint32_t t0,
                                                        int32_t steps) {
#if defined(__HIP_DEVICE_COMPILE__)  // (pop::const_entry, population.h)
  const auto& en = pop::const_entry(tab, active[blockIdx.y]);
  KParams p = en.kp;
  p.kc = kc;
  RollArgs a = en.a;
  a.t0 = t0;
  a.steps = steps;
  const float* __restrict__ packed = en.packed;
  ac_rollout_body<KIND, CTBR, MB>(*kc, p, packed, net, a);
#endif
}

}  // namespace

template <int AKIND, int MB>
hipError_t launch_pop_actor_rollout_inst(const KConsts<float>* kc, const pop::RollEntry* tab, const int32_t* active,
                                         int count, int n, bool ctbr, const ActorNet& net, uint32_t t0, int32_t steps,
                                         hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  constexpr int MAX_BYTES = 2 * arch::Layout{actor::MAX_H1 / 32, MB}.lds_bytes();  // (launch_actor_rollout_inst's rule)
  const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
  constexpr int KIND = AKIND == 1 ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
  const dim3 grid((n + 63) / 64, count), block(128);
  return with_bool(ctbr, [&](auto cb) {
    constexpr bool CB = decltype(cb)::value;
    if (const hipError_t e = lds_opt_in<&k_pop_ac_rollout<KIND, CB, MB>>(MAX_BYTES)) return e;
    return launch_lds<&k_pop_ac_rollout<KIND, CB, MB>>(grid, block, bytes, s, kc, tab, active, dn, t0, steps);
  });
}
template hipError_t launch_pop_actor_rollout_inst<AR_KIND, AR_MB>(const KConsts<float>*, const pop::RollEntry*,
                                                                  const int32_t*, int, int, bool, const ActorNet&,
                                                                  uint32_t, int32_t, hipStream_t);

template <int AKIND, int MB>
hipError_t launch_actor_rollout_inst(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                                     const float* packed, const RollArgs& a, hipStream_t s) {
  const actor::Net dn{net.nb1, net.actfn};
  // opted in once for the widest H1 of this MB (the table is per kernel, not per size), launched with this arch's
  constexpr int MAX_BYTES = 2 * arch::Layout{actor::MAX_H1 / 32, MB}.lds_bytes();
  const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
  constexpr int KIND = AKIND == 1 ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
  const dim3 grid((kp.n + 63) / 64), block(128);
  return with_bool(ctbr, [&](auto cb) {
    constexpr bool CB = decltype(cb)::value;
    if (const hipError_t e = lds_opt_in<&k_ac_rollout<KIND, CB, MB>>(MAX_BYTES)) return e;
    return launch_lds<&k_ac_rollout<KIND, CB, MB>>(grid, block, bytes, s, kc, kp, packed, dn, a);
  });
}
template hipError_t launch_actor_rollout_inst<AR_KIND, AR_MB>(const KConsts<float>*, const KParams&, bool,
                                                              const ActorNet&, const float*, const RollArgs&,
                                                              hipStream_t);

}  // namespace quadenv
#endif  // AR_DEPLOYED

#else  // the C entry points' object

namespace {

enum { CUR_T = 0, CUR_PENDING = 1, CUR_ARRIVED = 2 };

int rfail(int code, const char* m) { return set_error(code, m); }

// ---- pack: the value head zero-padded to four outputs (+ log_std), see the header
struct HeadArgs {
  const float *val_w, *val_b, *log_std;
  float* packed;
  int32_t h2;
  int64_t image;  // A
};
__device__ __forceinline__ void ac_head_body(const HeadArgs& a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nw = ACT * a.h2;
  if (idx < nw) a.packed[idx] = idx < a.h2 ? a.val_w[idx] : 0.f;
  else if (idx < nw + ACT) a.packed[idx] = idx == nw ? a.val_b[0] : 0.f;
  else if (idx < nw + 2 * ACT) a.packed[2 * a.image + (idx - nw - ACT)] = a.log_std[idx - nw - ACT];
}
__global__ void k_ac_head(HeadArgs a) { ac_head_body(a); }

// what the pack kernel reads for one net of the module: 1 the value net, its head the padded one k_ac_head left in the
// first floats of the image, 0 the policy net
__host__ __device__ inline QuadActorParams net_params(const QuadPolicyParams& p, const float* packed, int h2, int net) {
  return net ? QuadActorParams{p.vf_w0, p.vf_b0, p.vf_w1, p.vf_b1, packed, packed + ACT * h2}
             : QuadActorParams{p.pi_w0, p.pi_b0, p.pi_w1, p.pi_b1, p.act_w, p.act_b};
}

// The population forms of the pack's three launches (population.h): block (b, k) is block b of member active[k]'s
// launch; the member's entry is quad_policy_pack's (its parameters and its image), the arch comes with the launch
__global__ void k_pop_ac_head(const pop::PackEntry* __restrict__ tab, const int32_t* __restrict__ active, int32_t h2,
                              int64_t image) {
  const pop::PackEntry e = tab[active[blockIdx.y]];
  ac_head_body(HeadArgs{e.p.val_w, e.p.val_b, e.p.log_std, e.packed, h2, image});
}
__global__ void k_pop_ac_pack(const pop::PackEntry* __restrict__ tab, const int32_t* __restrict__ active, int32_t h1,
                              int32_t h2, int64_t image, int32_t net) {
  const pop::PackEntry e = tab[active[blockIdx.y]];
  actor::pack_body<arch::Layout, true, OBS>(net_params(e.p, e.packed, h2, net), h1, h2, e.packed + (net ? image : 0));
}

struct EpiArgs {  // QuadRolloutPost, flattened
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const float* terminal_obs;
  float* buf_rew;
  float* last_start;
  float* ep_ret;
  float* ep_len;
  double* stats;
  int32_t rows;
  float gamma;
};

// the input fragment of one row: features 8 h .. 8 h + 7 (zero past feature 11)
__device__ __forceinline__ void load_xb(const float* __restrict__ x, int row, bool ok, int h, float (&xb)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) xb[k] = ok && (h == 0 || k < 4) ? x[size_t(row) * OBS + 8 * h + k] : 0.f;
}

// finish step t - 1 for one tile (policy.hip's epilogue_tile): TimeLimit bootstrap where truncated and not
// terminated (the value net only when the tile holds such an env), reward row, last_start, episode statistics
// (accumulated in st[3] of the h == 0 lanes). Returns the env's new last_start.
template <int MB>
__device__ __forceinline__ float epilogue_tile(const float* __restrict__ Lc, const float* packed,
                                               const actor::Net& net, const EpiArgs& e, int env, bool ok, int h,
                                               size_t row, float st[3]) {
  bool term = false, trunc = false;
  float rew = 0.f, ret0 = 0.f, len0 = 0.f;
  if (ok) {
    term = e.terminated[env] != 0;
    trunc = e.truncated[env] != 0;
    rew = e.reward[env];
    ret0 = e.ep_ret[env];
    len0 = e.ep_len[env];
  }
  const bool timeout = ok && trunc && !term;
  float tv = 0.f;
  if (__any(timeout)) {
    float xb[8];
    load_xb(e.terminal_obs, env, ok, h, xb);
    tv = forward_v<MB>(Lc, packed, net, xb);
  }
  const bool done = term || trunc;
  if (ok && h == 0) {
    e.buf_rew[row + env] = reward_row(timeout, rew, e.gamma, tv);
    const float ret = ret0 + rew, len = len0 + 1.f;
    if (done) { st[0] += ret; st[1] += len; st[2] += 1.f; }
    e.ep_ret[env] = done ? 0.f : ret;
    e.ep_len[env] = done ? 0.f : len;
    e.last_start[env] = done ? 1.f : 0.f;
  }
  return done ? 1.f : 0.f;
}

// block-reduce the episode statistics into this block's slot (uncontended atomics)
__device__ void flush_stats(double* stats, float st[3]) {
  constexpr int WAVES = actor::ACT_BLK / 64;
  __shared__ float red[3][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    float v = st[j];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) red[j][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float s = 0.f;
    for (int w = 0; w < WAVES; w++) s += red[threadIdx.x][w];
    if (s != 0.f) atomicAdd(&stats[(blockIdx.x % QUAD_POLICY_STAT_SLOTS) * 3 + threadIdx.x], double(s));
  }
}

// Last block to arrive applies t_next / pending_next to the cursor (policy.hip's cursor_arrive: only reads of the
// cursor need ordering, the kernel boundary publishes the data).
__device__ void cursor_arrive(uint32_t* cursor, uint32_t t_next, uint32_t pending_next, bool set_t) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(&cursor[CUR_ARRIVED], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      cursor[CUR_ARRIVED] = 0u;
      if (set_t) cursor[CUR_T] = t_next;
      cursor[CUR_PENDING] = pending_next;
    }
  }
}

struct ActArgs {
  const float* obs;         // [N,12]
  float* act_env;           // [N,4] clipped
  float* act;               // [T,N,4] unclipped sample or NULL
  float* logp;              // [T,N] or NULL
  float* value;             // [T,N] or NULL
  float* obs_copy;          // [T,N,12] or NULL
  const float* last_start;  // [N] or NULL
  float* starts;            // [T,N] or NULL
  uint32_t* cursor;         // {t, pending, arrivals} or NULL
  int32_t rows;
  int32_t deterministic;
  uint64_t seed;
  uint64_t env_base;
  int32_t n;
  int32_t fused;            // epilogue of step t-1 + cursor advance
};

template <int MB>
__device__ __forceinline__ void ac_act_body(const float* __restrict__ packed, const actor::Net& net, const ActArgs& a,
                                            const EpiArgs& e) {
  extern __shared__ float lds[];
  const arch::Layout lay{net.nb1, MB};
  float* Lc = lds + lay.lds_floats();
  // the cursor is read before the first barrier; the last block to arrive rewrites it after every block's
  const uint32_t t = a.cursor ? a.cursor[CUR_T] : 0u;
  const bool pend = a.fused && a.cursor[CUR_PENDING] != 0u;
  {
    const int nv = lay.lds_floats() / 4;
    const float4* sa = reinterpret_cast<const float4*>(packed);
    const float4* sc = reinterpret_cast<const float4*>(packed + lay.floats());
    float4* da = reinterpret_cast<float4*>(lds);
    float4* dc = reinterpret_cast<float4*>(Lc);
    for (int k = threadIdx.x; k < nv; k += actor::ACT_BLK) { da[k] = sa[k]; dc[k] = sc[k]; }
    __syncthreads();
  }
  const uint32_t rows = uint32_t(a.rows);
  const size_t row0 = size_t(t % rows) * a.n;
  const size_t rowp = size_t((t + rows - 1u) % rows) * a.n;
  const float* log_std = packed + 2 * lay.floats();
  float lstd[ACT], sd[ACT];
#pragma unroll
  for (int k = 0; k < ACT; k++) { lstd[k] = log_std[k]; sd[k] = expf(lstd[k]); }
  float st[3] = {0.f, 0.f, 0.f};
  actor::act_tiles(a.n, [&](int env, bool ok, int h) {
    float ls = 0.f;
    if (pend) ls = epilogue_tile<MB>(Lc, packed, net, e, env, ok, h, rowp, st);
    else if (a.last_start && ok) ls = a.last_start[env];
    float xb[8], mean[ACT], val;
    load_xb(a.obs, env, ok, h, xb);
    forward_ac<MB>(lds, Lc, packed, net, xb, mean, val);
    if (!ok) return;
    if (a.obs_copy) {
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (h == 0 || k < 4) a.obs_copy[(row0 + env) * OBS + 8 * h + k] = xb[k];
    }
    if (h) return;  // one lane per env from here
    if (a.starts) a.starts[row0 + env] = ls;
    float act[ACT], ac[ACT], lp;
    sample_action(a.deterministic != 0, a.seed, a.env_base + uint64_t(env), t, mean, sd, lstd, act, ac, lp);
    reinterpret_cast<float4*>(a.act_env)[env] = make_float4(ac[0], ac[1], ac[2], ac[3]);
    if (a.act) reinterpret_cast<float4*>(a.act + row0 * ACT)[env] = make_float4(act[0], act[1], act[2], act[3]);
    if (a.logp) a.logp[row0 + env] = lp;
    if (a.value) a.value[row0 + env] = val;
  });
  if (a.fused) {
    if (pend) flush_stats(e.stats, st);
    cursor_arrive(a.cursor, t + 1u, 1u, true);
  }
}

template <int MB>
__global__ __launch_bounds__(actor::ACT_BLK) void k_ac_act(const float* __restrict__ packed, actor::Net net, ActArgs a,
                                                           EpiArgs e) {
  ac_act_body<MB>(packed, net, a, e);
}

// The population form of the bootstrap value (population.h): block (b, k) is block b of member active[k]'s
// quad_actor_critic_act(deterministic, rows = 1, value = out), FusedActorCritic.value
template <int MB>
__global__ __launch_bounds__(actor::ACT_BLK) void k_pop_ac_value(const pop::ValueEntry* __restrict__ tab,
                                                                 const int32_t* __restrict__ active, actor::Net net,
                                                                 int32_t n) {
  const pop::ValueEntry v = tab[active[blockIdx.y]];
  ActArgs a{};
  a.obs = v.obs; a.act_env = v.act_env; a.value = v.value;
  a.rows = 1; a.deterministic = 1; a.n = n;
  ac_act_body<MB>(v.packed, net, a, EpiArgs{});
}

template <int MB>
__global__ __launch_bounds__(actor::ACT_BLK) void k_ac_post(const float* __restrict__ packed, actor::Net net, EpiArgs e,
                                                            uint32_t* cursor, int32_t n) {
  extern __shared__ float lds[];
  if (cursor[CUR_PENDING] == 0u) return;  // grid-uniform: nothing to finish
  const uint32_t t = cursor[CUR_T], rows = uint32_t(e.rows);
  const arch::Layout lay{net.nb1, MB};
  actor::stage<actor::ACT_BLK>(lds, packed + lay.floats(), lay.lds_floats());  // the value image alone
  const size_t rowp = size_t((t + rows - 1u) % rows) * n;
  float st[3] = {0.f, 0.f, 0.f};
  actor::act_tiles(n, [&](int env, bool ok, int h) { epilogue_tile<MB>(lds, packed, net, e, env, ok, h, rowp, st); });
  flush_stats(e.stats, st);
  cursor_arrive(cursor, 0u, 0u, false);
}

// k_ac_act takes both images' LDS parts (up to 112.6 KB): every entry point opts the three forms in, once per
// device and for the widest H1 (dispatch.h), so packing an image is enough for the launches captured into a graph later
int opt_in() {
  constexpr int BYTES = 2 * arch::Layout{actor::MAX_H1 / 32, 8}.lds_bytes();
  return lds_opt_in<&k_ac_act<2>, &k_ac_act<4>, &k_ac_act<8>, &k_pop_ac_value<2>, &k_pop_ac_value<4>,
                    &k_pop_ac_value<8>>(BYTES) == hipSuccess
             ? QUAD_OK
             : rfail(QUAD_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
}

int ac_net_of(const QuadActorArch* a, ActorNet* out) { return actor::net_of(a, "actor-critic arch", false, out); }

EpiArgs epi_args(const QuadRolloutPost* p) {
  return EpiArgs{p->reward, p->terminated, p->truncated, p->terminal_obs, p->buf_rew, p->last_start,
                 p->ep_ret, p->ep_len, p->stats, p->rows, p->gamma};
}

int check_epi(const QuadRolloutPost* p) {
  if (!p->reward || !p->terminated || !p->truncated || !p->terminal_obs || !p->buf_rew || !p->last_start ||
      !p->ep_ret || !p->ep_len || !p->stats)
    return rfail(QUAD_EINVAL, "actor-critic rollout epilogue: NULL buffer");
  if (p->rows < 1) return rfail(QUAD_EINVAL, "actor-critic rollout epilogue: rows must be >= 1");
  return QUAD_OK;
}

template <int AKIND>
hipError_t launch_by_mb(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                        const float* packed, const RollArgs& a, hipStream_t s) {
  return with_mb(net.mb, [&](auto mb) {
    return launch_actor_rollout_inst<AKIND, decltype(mb)::value>(kc, kp, ctbr, net, packed, a, s);
  });
}

template <int AKIND>
hipError_t launch_deployed_by_mb(const KConsts<float>* kc, const KParams& kp, bool ctbr, const ActorNet& net,
                                 const float* packed, const RollArgs& a, const EstArgs& est, double est_dt,
                                 hipStream_t s) {
  return with_mb(net.mb, [&](auto mb) {
    return launch_actor_rollout_deployed_inst<AKIND, decltype(mb)::value>(kc, kp, ctbr, net, packed, a, est, est_dt, s);
  });
}

// quad_actor_rollout's argument checks and its flattened arguments (also quad_actor_rollout_deployed's)
int rollout_args(const QuadHandle* h, const QuadActorArch* arch_, const float* packed, const QuadRollout* r,
                 const char* who, ActorNet* net, RollArgs* out) {
  const std::string w(who);
  if (int rc = ac_net_of(arch_, net)) return rc;
  if (!h || !packed || !r) return fail(QUAD_EINVAL, w + ": handle/packed/rollout is NULL");
  if (!r->obs_copy || !r->actions || !r->log_prob || !r->value || !r->episode_starts || !r->rewards ||
      !r->last_obs || !r->last_start || !r->ep_ret || !r->ep_len || !r->stats)
    return fail(QUAD_EINVAL, w + ": NULL buffer");
  if (r->rows < 1 || r->steps < 1 || r->t0 < 0) return fail(QUAD_EINVAL, w + ": rows, steps >= 1, t0 >= 0");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(r->actions) |
       reinterpret_cast<uintptr_t>(r->obs_copy) | reinterpret_cast<uintptr_t>(r->last_obs)) & 15u)
    return fail(QUAD_EINVAL, w + ": packed, actions, obs_copy and last_obs must be 16-byte aligned");
  if (h->cfg.env_kind != QUAD_ENV_HOVER && h->cfg.env_kind != QUAD_ENV_TRAJ)
    return fail(QUAD_EINVAL, w + ": env_kind must be HOVER or TRAJ");
  if (h->cfg.wrapper != QUAD_WRAP_NONE && h->cfg.wrapper != QUAD_WRAP_CTBR)
    return fail(QUAD_EINVAL, w + ": the policy takes 12-D obs (wrapper NONE or CTBR)");
  if (!h->cfg.auto_reset) return fail(QUAD_EINVAL, w + ": the handle needs auto_reset = 1");
  *out = RollArgs{r->obs_copy, r->actions, r->log_prob, r->value, r->episode_starts, r->rewards, r->last_obs,
                  r->last_start, r->ep_ret, r->ep_len, r->stats, uint32_t(r->rows), uint32_t(r->t0), r->steps,
                  r->deterministic, r->seed, r->gamma};
  return QUAD_OK;
}

template <int AKIND>
hipError_t launch_pop_by_mb(const KConsts<float>* kc, const pop::RollEntry* tab, const int32_t* active, int count, int n,
                            bool ctbr, const ActorNet& net, uint32_t t0, int32_t steps, hipStream_t s) {
  return with_mb(net.mb, [&](auto mb) {
    return launch_pop_actor_rollout_inst<AKIND, decltype(mb)::value>(kc, tab, active, count, n, ctbr, net, t0, steps, s);
  });
}

template <int AKIND>
hipError_t launch_pop_deployed_by_mb(const KConsts<float>* kc, const pop::RollEntry* tab, const pop::EstEntry* etab,
                                     const int32_t* active, int count, int n, bool ctbr, const ActorNet& net, uint32_t t0,
                                     int32_t steps, hipStream_t s) {
  return with_mb(net.mb, [&](auto mb) {
    return launch_pop_actor_rollout_deployed_inst<AKIND, decltype(mb)::value>(kc, tab, etab, active, count, n, ctbr, net,
                                                                              t0, steps, s);
  });
}

}  // namespace

// ---- the population launches of this file's kernels (population.h); `arch` is one quad_pop_create_arch checked
int pop::launch_pop_ac_pack(const QuadActorArch& arch, const PackEntry* tab, const int32_t* active, int count,
                            hipStream_t s) {
  if (int rc = opt_in()) return rc;
  const arch::Layout lay{arch.h1 / 32, arch.h2 / 32};
  const int64_t A = lay.floats();
  hipLaunchKernelGGL(k_pop_ac_head, dim3((ACT * arch.h2 + 2 * ACT + 255) / 256, count), dim3(256), 0, s, tab, active,
                     arch.h2, A);
  if (hipGetLastError() != hipSuccess) return rfail(QUAD_EHIP, "k_pop_ac_head launch failed");
  for (int net = 1; net >= 0; net--) {  // the value half from the padded head, then the policy half over it
    hipLaunchKernelGGL(k_pop_ac_pack, dim3(actor::pack_blocks(lay), count), dim3(256), 0, s, tab, active, arch.h1,
                       arch.h2, A, net);
    if (hipGetLastError() != hipSuccess) return rfail(QUAD_EHIP, "k_pop_ac_pack launch failed");
  }
  return QUAD_OK;
}

int pop::launch_pop_ac_value(const QuadActorArch& arch, const ValueEntry* tab, const int32_t* active, int count, int n,
                             hipStream_t s) {
  if (int rc = opt_in()) return rc;
  const actor::Net net{arch.h1 / 32, arch.activation};
  const hipError_t err = with_mb(arch.h2 / 32, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
    hipLaunchKernelGGL((k_pop_ac_value<MB>), dim3(actor::act_grid(n).x, count), dim3(actor::ACT_BLK), bytes, s, tab,
                       active, net, n);
    return hipGetLastError();
  });
  return err == hipSuccess ? QUAD_OK : rfail(QUAD_EHIP, "k_pop_ac_value launch failed");
}

hipError_t pop::launch_pop_ac_rollout(const QuadActorArch& arch, const KConsts<float>* kc, const RollEntry* tab,
                                      const int32_t* active, int count, int n, int env_kind, bool ctbr, uint32_t t0,
                                      int32_t steps, hipStream_t s) {
  const ActorNet net{arch.h1 / 32, arch.h2 / 32, arch.activation};
  return env_kind == QUAD_ENV_TRAJ ? launch_pop_by_mb<1>(kc, tab, active, count, n, ctbr, net, t0, steps, s)
                                   : launch_pop_by_mb<0>(kc, tab, active, count, n, ctbr, net, t0, steps, s);
}

hipError_t pop::launch_pop_ac_rollout_deployed(const QuadActorArch& arch, const KConsts<float>* kc, const RollEntry* tab,
                                               const EstEntry* etab, const int32_t* active, int count, int n,
                                               int env_kind, bool ctbr, uint32_t t0, int32_t steps, hipStream_t s) {
  const ActorNet net{arch.h1 / 32, arch.h2 / 32, arch.activation};
  return env_kind == QUAD_ENV_TRAJ
             ? launch_pop_deployed_by_mb<1>(kc, tab, etab, active, count, n, ctbr, net, t0, steps, s)
             : launch_pop_deployed_by_mb<0>(kc, tab, etab, active, count, n, ctbr, net, t0, steps, s);
}

}  // namespace quadenv

using namespace quadenv;

extern "C" {

int64_t quad_actor_critic_packed_floats(const QuadActorArch* a) {
  ActorNet net;
  if (ac_net_of(a, &net)) return -1;
  return 2 * arch::Layout{net.nb1, net.mb}.floats() + ACT;
}

int quad_actor_critic_pack(const QuadActorArch* a, const QuadPolicyParams* p, float* packed, void* stream) {
  ActorNet net;
  if (int rc = ac_net_of(a, &net)) return rc;
  if (!p || !packed) return rfail(QUAD_EINVAL, "quad_actor_critic_pack: params/packed is NULL");
  if (!p->pi_w0 || !p->pi_b0 || !p->pi_w1 || !p->pi_b1 || !p->act_w || !p->act_b || !p->vf_w0 || !p->vf_b0 ||
      !p->vf_w1 || !p->vf_b1 || !p->val_w || !p->val_b || !p->log_std)
    return rfail(QUAD_EINVAL, "quad_actor_critic_pack: a parameter pointer is NULL");
  if (reinterpret_cast<uintptr_t>(packed) & 15u)
    return rfail(QUAD_EINVAL, "quad_actor_critic_pack: packed must be 16-byte aligned");
  if (int rc = opt_in()) return rc;
  const arch::Layout lay{net.nb1, net.mb};
  const int64_t A = lay.floats();
  const int h2 = net.mb * 32;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_ac_head, dim3((ACT * h2 + 2 * ACT + 255) / 256), dim3(256), 0, s,
                     HeadArgs{p->val_w, p->val_b, p->log_std, packed, h2, A});
  if (hipGetLastError() != hipSuccess) return rfail(QUAD_EHIP, "k_ac_head launch failed");
  if (actor::launch_pack<arch::Layout, true, OBS>(lay, net_params(*p, packed, h2, 1), packed + A, s) != hipSuccess)
    return rfail(QUAD_EHIP, "k_actor_pack (value net) launch failed");
  if (actor::launch_pack<arch::Layout, true, OBS>(lay, net_params(*p, packed, h2, 0), packed, s) != hipSuccess)
    return rfail(QUAD_EHIP, "k_actor_pack (policy net) launch failed");
  return QUAD_OK;
}

int quad_actor_critic_act(const QuadActorArch* arch_, const float* packed, const QuadPolicyAct* s, int32_t n,
                          void* stream) {
  ActorNet net;
  if (int rc = ac_net_of(arch_, &net)) return rc;
  if (!packed || !s || !s->obs || !s->actions_env) return rfail(QUAD_EINVAL, "quad_actor_critic_act: NULL argument");
  if (n <= 0) return rfail(QUAD_EINVAL, "quad_actor_critic_act: n must be > 0");
  if (s->rows < 1) return rfail(QUAD_EINVAL, "quad_actor_critic_act: rows must be >= 1");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(s->actions_env) |
       reinterpret_cast<uintptr_t>(s->actions)) & 15u)
    return rfail(QUAD_EINVAL, "quad_actor_critic_act: packed and action buffers must be 16-byte aligned");
  EpiArgs e{};
  if (s->epilogue) {
    if (!s->cursor) return rfail(QUAD_EINVAL, "quad_actor_critic_act: a fused epilogue needs the cursor");
    if (int rc = check_epi(s->epilogue)) return rc;
    if (s->epilogue->rows != s->rows) return rfail(QUAD_EINVAL, "quad_actor_critic_act: epilogue rows != rows");
    e = epi_args(s->epilogue);
  }
  if (int rc = opt_in()) return rc;
  const ActArgs a{s->obs, s->actions_env, s->actions, s->log_prob, s->value, s->obs_copy, s->last_start,
                  s->episode_starts, s->cursor, s->rows, s->deterministic, s->seed, s->env_id_base, n,
                  s->epilogue ? 1 : 0};
  const hipError_t err = with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const int bytes = 2 * arch::Layout{net.nb1, MB}.lds_bytes();
    hipLaunchKernelGGL((k_ac_act<MB>), actor::act_grid(n), dim3(actor::ACT_BLK), bytes, static_cast<hipStream_t>(stream),
                       packed, actor::Net{net.nb1, net.actfn}, a, e);
    return hipGetLastError();
  });
  return err == hipSuccess ? QUAD_OK : rfail(QUAD_EHIP, "k_ac_act launch failed");
}

int quad_actor_critic_post(const QuadActorArch* arch_, const float* packed, const QuadRolloutPost* p, uint32_t* cursor,
                           int32_t n, void* stream) {
  ActorNet net;
  if (int rc = ac_net_of(arch_, &net)) return rc;
  if (!packed || !p || !cursor) return rfail(QUAD_EINVAL, "quad_actor_critic_post: NULL argument");
  if (n <= 0) return rfail(QUAD_EINVAL, "quad_actor_critic_post: n must be > 0");
  if (reinterpret_cast<uintptr_t>(packed) & 15u)
    return rfail(QUAD_EINVAL, "quad_actor_critic_post: packed must be 16-byte aligned");
  if (int rc = check_epi(p)) return rc;
  const hipError_t err = with_mb(net.mb, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const int bytes = arch::Layout{net.nb1, MB}.lds_bytes();  // one image, <= 64 KB: no opt-in
    hipLaunchKernelGGL((k_ac_post<MB>), actor::act_grid(n), dim3(actor::ACT_BLK), bytes, static_cast<hipStream_t>(stream),
                       packed, actor::Net{net.nb1, net.actfn}, epi_args(p), cursor, n);
    return hipGetLastError();
  });
  return err == hipSuccess ? QUAD_OK : rfail(QUAD_EHIP, "k_ac_post launch failed");
}

int quad_actor_rollout(QuadHandle* h, const QuadActorArch* arch_, const float* packed, const QuadRollout* r,
                       void* stream) {
  ActorNet net;
  RollArgs a;
  if (int rc = rollout_args(h, arch_, packed, r, "quad_actor_rollout", &net, &a)) return rc;
  DeviceGuard g(h->device);
  const bool ctbr = h->cfg.wrapper == QUAD_WRAP_CTBR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = h->cfg.env_kind == QUAD_ENV_TRAJ ? launch_by_mb<1>(h->kdev, h->kp, ctbr, net, packed, a, s)
                                                        : launch_by_mb<0>(h->kdev, h->kp, ctbr, net, packed, a, s);
  return e == hipSuccess ? QUAD_OK : hip_fail(e, "k_ac_rollout launch");
}

int quad_actor_rollout_deployed(QuadHandle* h, const QuadActorArch* arch_, const float* packed, const QuadRollout* r,
                                const QuadVelEst* est, double est_dt, void* stream) {
  ActorNet net;
  RollArgs a;
  if (int rc = rollout_args(h, arch_, packed, r, "quad_actor_rollout_deployed", &net, &a)) return rc;
  if (!est) return fail(QUAD_EINVAL, "quad_actor_rollout_deployed: est is NULL");
  if (int rc = check_est(est, "quad_actor_rollout_deployed")) return rc;
  if (!est->state) return fail(QUAD_EINVAL, "quad_actor_rollout_deployed: the estimator state block is required");
  if ((reinterpret_cast<uintptr_t>(est->state) | reinterpret_cast<uintptr_t>(est->alpha)) & 7u)
    return fail(QUAD_EINVAL, "quad_actor_rollout_deployed: est->state and est->alpha must be 8-byte aligned");
  if (!(est_dt > 0.0) || !std::isfinite(est_dt))
    return fail(QUAD_EINVAL, "quad_actor_rollout_deployed: est_dt must be > 0 and finite");
  DeviceGuard g(h->device);
  const bool ctbr = h->cfg.wrapper == QUAD_WRAP_CTBR;
  const EstArgs ea{est->alpha, est->alpha_all, est->max_dt, est->state};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = h->cfg.env_kind == QUAD_ENV_TRAJ
                           ? launch_deployed_by_mb<1>(h->kdev, h->kp, ctbr, net, packed, a, ea, est_dt, s)
                           : launch_deployed_by_mb<0>(h->kdev, h->kp, ctbr, net, packed, a, ea, est_dt, s);
  return e == hipSuccess ? QUAD_OK : hip_fail(e, "k_ac_rollout_deployed launch");
}

}  // extern "C"
#endif
