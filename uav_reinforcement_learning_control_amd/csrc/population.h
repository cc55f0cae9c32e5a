// population.h -- PPO populations in lock-step launches (quad_pop_*, include/quadenv.h): the device
// table entries of each kernel family and the host launchers the translation units export. A population
// kernel is the single kernel's body behind one more grid dimension: block (.., k) runs member active[k],
// whose argument struct it reads from the family's device table (population.hip builds the tables once).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "env_tiles.h"
#include "learner.h"
#include "learner_arch.h"
#include "policy_episode.h"
#include "rollout.h"

namespace quadenv {
namespace pop {

// A table entry seen through the constant address space (device code only). A population table is written by
// the host before any launch and never while one runs, so its entries are invariant for a kernel, exactly as
// its kernel arguments are; the constant address space tells the compiler so, and it may then re-issue an
// entry's scalar loads where it would otherwise hold the values in registers or spill them. Read as plain
// global loads into locals, the one-tile forms of k_pop_rollout spilled 4-28 bytes per lane more than k_rollout
// (DESIGN 18). The register-tight kernels (rollout, policy episode) read their entry this way; the host pass
// has no copy from an address-space-qualified struct, so their bodies are device-only.
#if defined(__HIP_DEVICE_COMPILE__)
template <class Entry>
__device__ __forceinline__ const __attribute__((address_space(4))) Entry& const_entry(const Entry* tab, int32_t m) {
  typedef const __attribute__((address_space(4))) Entry* CEntry;
  return *(CEntry)(uintptr_t)(tab + m);
}
#endif

// ---- rollout (rollout.hip): k_rollout's arguments, per member; t0 / steps come with the launch
struct RollEntry {
  KParams kp;  // kc unused: the launch passes the shared constant block as its noalias argument
  const float* packed;
  RollArgs a;
};
hipError_t launch_pop_rollout(const KConsts<float>* kc, const RollEntry* tab, const int32_t* active, int count, int n,
                              int env_kind, bool ctbr, bool spec, uint32_t t0, int32_t steps, hipStream_t s);

// ---- GAE (quadenv.hip): k_gae's arguments
struct GaeEntry {
  const float *rew, *val, *starts, *last_val, *dones;
  float *adv, *ret;
  float gamma, lam;
};
hipError_t launch_pop_gae(const GaeEntry* tab, const int32_t* active, int count, int T, int n, hipStream_t s);

// ---- policy image and bootstrap value (policy.hip)
struct PackEntry {
  QuadPolicyParams p;
  float* packed;
};
struct ValueEntry {  // quad_policy_act(deterministic, rows = 1, value = out): FusedPolicy.value
  const float* packed;
  const float* obs;
  float* act_env;
  float* value;
};
int launch_pop_pack(const PackEntry* tab, const int32_t* active, int count, hipStream_t s);
int launch_pop_value(const ValueEntry* tab, const int32_t* active, int count, int n, hipStream_t s);

// ---- learner (learner.hip, learner_x3.hip). The GArgs entry of a member holds the epoch's bases: idx = the
// permutation, adv_part = the [n_minibatches][QUAD_ADV_SUM_DOUBLES] sums (NULL without normalization); the
// gradient launch of minibatch `slot` advances both. RArgs.stats likewise is the [n_minibatches][4] base.
struct LearnerTables {  // device
  lrn::GArgs* g = nullptr;
  lrn::RArgs* r = nullptr;
  lrn::AdamArgs* a = nullptr;
};
// validate member `m`'s learner arguments and fill entry `i` of the host images (QUAD_EINVAL + message)
int fill_learner(const QuadPopMember& m, int i, int32_t batch, int32_t normalize, lrn::GArgs* g, lrn::RArgs* r,
                 lrn::AdamArgs* a);
int64_t learner_workspace_bytes(const QuadAdam* adam, int32_t batch);
int launch_pop_permutation(const lrn::GArgs* tab, const int32_t* active, int count, int64_t n, const uint64_t* seeds,
                           hipStream_t s);
int launch_pop_adv_stats_epoch(const lrn::GArgs* tab, const int32_t* active, int count, int n_minibatches,
                               hipStream_t s);
int launch_pop_reduce(const lrn::RArgs* rtab, const int32_t* active, int count, int slot, hipStream_t s);
int launch_pop_clip_adam(const lrn::AdamArgs* atab, const int32_t* active, int count, int nblocks, hipStream_t s);
// fill_learner's checks and the entries every family's learner shares (`who` prefixes the messages): the GArgs the
// permutation and the advantage sums read, the Adam entry with its gradient-norm partials at workspace + adam_offset
int fill_member(const char* who, const QuadPopMember& m, int i, int32_t batch, int32_t normalize, int64_t adam_offset,
                lrn::GArgs* g, lrn::AdamArgs* a);
int64_t adam_partials_bytes(const QuadAdam* adam);  // 0: the QuadAdam is invalid

// ---- the general family (actor_rollout.hip, actor_arch.hip): the same entries -- a member's image is
// quad_actor_critic_pack's, whose first quad_actor_packed_floats floats are the policy net's episode image -- and the
// population's arch with every launch
int launch_pop_ac_pack(const QuadActorArch& arch, const PackEntry* tab, const int32_t* active, int count, hipStream_t s);
int launch_pop_ac_value(const QuadActorArch& arch, const ValueEntry* tab, const int32_t* active, int count, int n,
                        hipStream_t s);
hipError_t launch_pop_ac_rollout(const QuadActorArch& arch, const KConsts<float>* kc, const RollEntry* tab,
                                 const int32_t* active, int count, int n, int env_kind, bool ctbr, uint32_t t0,
                                 int32_t steps, hipStream_t s);
// obs_mode: QUAD_OBS_ENV, or QUAD_OBS_DEPLOYED for a quad_pop_create_deployed population (every entry's estimator
// arguments are then read)
hipError_t launch_pop_actor_episode(const QuadActorArch& arch, const KConsts<float>* kc, const PopEpisodeEntry* tab,
                                    const int32_t* active, int count, int n, int env_kind, bool ctbr, int obs_mode,
                                    hipStream_t s);

// ---- the deployed observation (actor_rollout.hip's AR_DEPLOYED objects): quad_actor_rollout_deployed's
// estimator arguments, per member, in a table of their own beside the RollEntry table (which every rollout kernel of
// both families reads, and which keeps its size): members may differ in alpha_all, their alpha arrays and max_dt
struct EstEntry {
  EstArgs est;
  double est_dt;
};
hipError_t launch_pop_ac_rollout_deployed(const QuadActorArch& arch, const KConsts<float>* kc, const RollEntry* tab,
                                          const EstEntry* etab, const int32_t* active, int count, int n, int env_kind,
                                          bool ctbr, uint32_t t0, int32_t steps, hipStream_t s);

}  // namespace pop

namespace lrna {
// The general learner's minibatch gradient (learner_arch.hip). A member's entry is quad_ppo_arch_grad's Args with the
// epoch's bases, as the GArgs entry above: g (fill_member's) with idx = the permutation and adv_part = the sums of
// every minibatch, stats = the [n_minibatches][4] base; the launch of minibatch `slot` advances the three
Args pop_entry(const QuadActorArch& arch, const lrn::GArgs& g, const QuadPopMember& m, int32_t batch);
int launch_pop_grad(const QuadActorArch& arch, int32_t batch, const Args* tab, const int32_t* active, int count,
                    int slot, hipStream_t s);
}  // namespace lrna

namespace lrn {
// k_x3_prep's W2 split + k_ppo_grad_x3_sep for every active member (learner_x3.hip); nb = layout_both(batch).nb
int launch_pop_grad_x3(const GArgs* tab, const int32_t* active, int count, int slot, int nb, hipStream_t s);
}  // namespace lrn

}  // namespace quadenv
