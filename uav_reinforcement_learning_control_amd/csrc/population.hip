// population.hip -- PPO populations in lock-step launches (quad_pop_*, include/quadenv.h): host
// side only. quad_pop_create validates P members that share every shape, builds one device table per kernel
// family (each entry is the argument struct the single kernel takes by value) and uploads them once;
// quad_pop_subset uploads a list of member indices once. A launch call then passes (table, subset list,
// count) to the family's population kernel (rollout.hip, policy.hip, quadenv.hip, learner.hip,
// learner_x3.hip): no allocation, no copy, no synchronization, so it is stream-ordered and graph-capturable.
// quad_pop_create_arch builds the same tables for members of one arch of the general family; the launch
// calls then go to that family's population kernels (actor_rollout.hip, actor_arch.hip, learner_arch.hip).
// quad_pop_create_deployed adds the estimator table of the deployed rollout; its (128, 128) ReLU populations
// pair the family's actor tables with the 128-128 ReLU learner's, as a single deployed learner of that net does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/quadenv.h"
#include "handle.h"
#include "population.h"

using namespace quadenv;
using namespace quadenv::pop;

struct QuadPop {
  int32_t P = 0, n = 0, rows = 0, batch = 0, nmb = 0, normalize = 0;
  int device = 0;
  int32_t env_kind = 0;
  bool ctbr = false, spec = false;
  const KConsts<float>* kc = nullptr;  // member 0's constant block (every member's is equal)
  int32_t nb = 0, adam_nblocks = 0;
  RollEntry* roll = nullptr;
  GaeEntry* gae = nullptr;
  PackEntry* pack = nullptr;
  ValueEntry* value = nullptr;
  LearnerTables lt;
  bool fam_actor = false;      // pack, rollout, value and episode are the general family's (arch): quad_pop_create_arch
                               // and quad_pop_create_deployed
  bool fam_learner = false;    // the gradient is the general learner's (ga; lt.r unused): every arch of those two but
                               // the deployed (128, 128) ReLU one, whose gradient is quad_ppo_grad's (lt.r)
  bool deployed = false;       // quad_pop_create_deployed: est, the rollout and the episodes in QUAD_OBS_DEPLOYED mode
  QuadActorArch arch{};
  EstEntry* est = nullptr;     // the deployed rollout's estimator table, by member
  lrna::Args* ga = nullptr;    // the general learner's gradient table
  std::vector<const float*> packed;  // the members' packed images (quad_pop_attach_eval)
  PopEpisodeEntry* eval = nullptr;   // the evaluation table, once attached
  const KConsts<float>* eval_kc = nullptr;
  int32_t eval_n = 0, eval_kind = 0;
  bool eval_ctbr = false, eval_spec = false;
  std::vector<char> eval_ok;         // per member: the table holds an evaluation entry
  struct Subset {
    int32_t* dev;
    int32_t count;
    std::vector<int32_t> members;  // host copy
  };
  std::vector<Subset> subsets;
};

namespace {

constexpr int32_t POP_MAX_MEMBERS = 65535;  // gridDim.y / gridDim.z
constexpr int32_t POP_MAX_BATCH = 8192;  // k_ppo_grad_x3_sep's limit: 2 nb <= X3_BLOCKS

int pfail(const std::string& m) { return set_error(QUAD_EINVAL, m.c_str()); }
int hfail(const char* what, hipError_t e) {
  return set_error(QUAD_EHIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

// two handles agree on what a population shares: kind, wrapper, constants (bit for bit), env count and device
bool same_envs(const QuadHandle* a, const QuadHandle* b) {
  return a->cfg.env_kind == b->cfg.env_kind && a->cfg.wrapper == b->cfg.wrapper && a->n == b->n &&
         a->device == b->device && a->spec == b->spec && std::memcmp(&a->kh, &b->kh, sizeof(KConsts<float>)) == 0;
}

template <class T>
hipError_t upload(T** dev, const void* host, size_t bytes) {
  if (hipError_t e = hipMalloc(reinterpret_cast<void**>(dev), bytes)) return e;
  return hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
}

void release(QuadPop* p) {
  if (!p) return;
  DeviceGuard g(p->device);
  (void)hipFree(p->roll);
  (void)hipFree(p->gae);
  (void)hipFree(p->pack);
  (void)hipFree(p->value);
  (void)hipFree(p->lt.g);
  (void)hipFree(p->lt.r);
  (void)hipFree(p->lt.a);
  (void)hipFree(p->ga);
  (void)hipFree(p->est);
  (void)hipFree(p->eval);
  for (auto& s : p->subsets) (void)hipFree(s.dev);
  delete p;
}

int add_subset(QuadPop* p, const int32_t* members, int32_t count, int32_t* id) {
  if (!members || count < 1) return pfail("quad_pop_subset: the subset is empty");
  if (count > p->P) return pfail("quad_pop_subset: more entries than members");
  std::vector<char> seen(size_t(p->P), 0);
  for (int32_t k = 0; k < count; k++) {
    if (members[k] < 0 || members[k] >= p->P) return pfail("quad_pop_subset: member index out of range");
    if (seen[size_t(members[k])]) return pfail("quad_pop_subset: duplicate member");
    seen[size_t(members[k])] = 1;
  }
  DeviceGuard g(p->device);
  int32_t* dev = nullptr;
  if (hipError_t e = upload(&dev, members, size_t(count) * sizeof(int32_t))) {
    (void)hipFree(dev);
    return hfail("quad_pop_subset", e);
  }
  p->subsets.push_back(QuadPop::Subset{dev, count, std::vector<int32_t>(members, members + count)});
  if (id) *id = int32_t(p->subsets.size()) - 1;
  return QUAD_OK;
}

// the subset of a launch call, or NULL (error set)
const QuadPop::Subset* subset_of(QuadPop* p, int32_t id, const char* what) {
  if (!p) {
    pfail(std::string(what) + ": population is NULL");
    return nullptr;
  }
  if (id < 0 || size_t(id) >= p->subsets.size()) {
    pfail(std::string(what) + ": unknown subset id");
    return nullptr;
  }
  return &p->subsets[size_t(id)];
}

// the 13 Adam tensors of an arch's module hold these element counts (in any order)
bool adam_fits(const QuadAdam& ad, const QuadActorArch& a) {
  std::vector<int32_t> want = {a.h1 * 12, a.h1, a.h2 * a.h1, a.h2, 4 * a.h2, 4, a.h1 * 12, a.h1, a.h2 * a.h1, a.h2,
                               a.h2, 1, 4};
  if (ad.count != int32_t(want.size())) return false;
  std::vector<int32_t> got(ad.numel, ad.numel + ad.count);
  std::sort(want.begin(), want.end());
  std::sort(got.begin(), got.end());
  return want == got;
}

// the gradient-norm partials follow the general learner's workspace
int64_t arch_adam_offset(const QuadActorArch& a, int32_t batch) { return lrna::up16(lrna::layout_of(a.h1, a.h2, batch).bytes); }

bool is_128_relu(const QuadActorArch& a) { return a.h1 == 128 && a.h2 == 128 && a.activation == QUAD_ACTFN_RELU; }

// quad_actor_rollout_deployed's estimator checks on member i's QuadPopDeploy
int check_deploy(const std::string& who, const QuadPopDeploy& d) {
  if (int rc = check_est(&d.est, who.c_str())) return rc;
  if (!d.est.state) return pfail(who + ": the estimator state block is required");
  if ((reinterpret_cast<uintptr_t>(d.est.state) | reinterpret_cast<uintptr_t>(d.est.alpha)) & 7u)
    return pfail(who + ": est.state and est.alpha must be 8-byte aligned");
  if (!(d.est_dt > 0.0) || !std::isfinite(d.est_dt)) return pfail(who + ": est_dt must be > 0 and finite");
  return QUAD_OK;
}

// quad_pop_create (arch == NULL: the 128-128 ReLU kernels), quad_pop_create_arch (the general family's) and
// quad_pop_create_deployed (fn names it; deploy: its estimators, one per member)
int create(const char* fn_, const QuadActorArch* arch, const QuadPopMember* members, const QuadPopDeploy* deploy,
           int32_t P, int32_t batch, int32_t normalize_advantage, QuadPop** out) {
  const std::string fn = fn_;
  const bool fam_learner = arch && !(deploy && is_128_relu(*arch));
  if (!members || !out) return pfail(fn + ": members / out is NULL");
  if (P < 1) return pfail(fn + ": P must be >= 1");
  if (P > POP_MAX_MEMBERS) return pfail(fn + ": P must be <= 65535 (the member is a grid y / z coordinate)");
  if (batch < 1 || batch > POP_MAX_BATCH)
    return pfail(fn + ": need 1 <= batch <= 8192 (the separate-block gradient form's limit)");
  if (!fam_learner && quad_ppo_grad_form() != 1) return pfail(fn + ": only the bf16x3 gradient has a population form");
  std::vector<lrna::Args> ga(fam_learner ? static_cast<size_t>(P) : 0);
  std::vector<EstEntry> est(deploy ? static_cast<size_t>(P) : 0);
  std::vector<RollEntry> roll(static_cast<size_t>(P));
  std::vector<GaeEntry> gae(static_cast<size_t>(P));
  std::vector<PackEntry> pack(static_cast<size_t>(P));
  std::vector<ValueEntry> value(static_cast<size_t>(P));
  std::vector<lrn::GArgs> gt(static_cast<size_t>(P));
  std::vector<lrn::RArgs> rt(static_cast<size_t>(P));
  std::vector<lrn::AdamArgs> at(static_cast<size_t>(P));
  const QuadHandle* v0 = nullptr;
  for (int32_t i = 0; i < P; i++) {
    const QuadPopMember& m = members[i];
    const QuadRollout& r = m.rollout;
    const std::string who = fn + ": member " + std::to_string(i) + ": ";
    if (!m.env || !m.packed) return pfail(who + "env / packed is NULL");
    if (!r.obs_copy || !r.actions || !r.log_prob || !r.value || !r.episode_starts || !r.rewards || !r.last_obs ||
        !r.last_start || !r.ep_ret || !r.ep_len || !r.stats || !m.last_values || !m.scratch_actions)
      return pfail(who + "a rollout buffer is NULL");
    if (r.rows < 1) return pfail(who + "rows must be >= 1");
    if ((reinterpret_cast<uintptr_t>(m.packed) | reinterpret_cast<uintptr_t>(r.actions) |
         reinterpret_cast<uintptr_t>(r.obs_copy) | reinterpret_cast<uintptr_t>(r.last_obs) |
         reinterpret_cast<uintptr_t>(m.scratch_actions)) & 15u)
      return pfail(who + "packed, actions, obs_copy, last_obs and scratch_actions must be 16-byte aligned");
    const QuadHandle* v = m.env;
    if (v->cfg.env_kind != QUAD_ENV_HOVER && v->cfg.env_kind != QUAD_ENV_TRAJ)
      return pfail(who + "env_kind must be HOVER or TRAJ");
    if (v->cfg.wrapper != QUAD_WRAP_NONE && v->cfg.wrapper != QUAD_WRAP_CTBR)
      return pfail(who + "the policy takes 12-D obs (wrapper NONE or CTBR)");
    if (!v->cfg.auto_reset) return pfail(who + "the handle needs auto_reset = 1");
    if (i == 0) v0 = v;
    if (!same_envs(v, v0)) return pfail(who + "env kind, wrapper, constants, env count or device differ from member 0's");
    if (r.rows != members[0].rollout.rows) return pfail(who + "rows differ from member 0's");
    const int64_t total = int64_t(r.rows) * v->n;
    if (total % batch != 0) return pfail(who + "rows x envs is not a multiple of the minibatch");
    if (total / batch > 65535) return pfail(who + "more than 65,535 minibatches per epoch");
    roll[size_t(i)] = RollEntry{v->kp, m.packed,
                                RollArgs{r.obs_copy, r.actions, r.log_prob, r.value, r.episode_starts, r.rewards,
                                         r.last_obs, r.last_start, r.ep_ret, r.ep_len, r.stats, uint32_t(r.rows), 0u, 0,
                                         r.deterministic, r.seed, r.gamma}};
    gae[size_t(i)] = GaeEntry{r.rewards, r.value, r.episode_starts, m.last_values, r.last_start,
                              m.advantages, m.returns, r.gamma, m.gae_lambda};
    pack[size_t(i)] = PackEntry{m.params, m.packed};
    value[size_t(i)] = ValueEntry{m.packed, r.last_obs, m.scratch_actions, m.last_values};
    if (deploy) {
      const QuadPopDeploy& d = deploy[i];
      if (int rc = check_deploy(fn + ": member " + std::to_string(i), d)) return rc;
      est[size_t(i)] = EstEntry{EstArgs{d.est.alpha, d.est.alpha_all, d.est.max_dt, d.est.state}, d.est_dt};
    }
    if (fam_learner) {
      if (int rc = fill_member(fn.c_str(), m, i, batch, normalize_advantage, arch_adam_offset(*arch, batch), gt.data(),
                               at.data()))
        return rc;
      ga[size_t(i)] = lrna::pop_entry(*arch, gt[size_t(i)], m, batch);
    } else if (int rc = fill_learner(m, i, batch, normalize_advantage, gt.data(), rt.data(), at.data())) {
      return rc;
    }
    if (arch && !adam_fits(m.adam, *arch)) return pfail(who + "the Adam tensor sizes are not the arch's");
    if (m.adam.count != members[0].adam.count ||
        std::memcmp(m.adam.numel, members[0].adam.numel, sizeof(int32_t) * size_t(m.adam.count)) != 0)
      return pfail(who + "Adam tensor sizes differ from member 0's");
  }
  QuadPop* p = new (std::nothrow) QuadPop();
  if (!p) return set_error(QUAD_ENOMEM, "quad_pop_create: out of host memory");
  p->P = P; p->n = v0->n; p->rows = members[0].rollout.rows; p->batch = batch;
  p->nmb = int32_t(int64_t(p->rows) * p->n / batch);
  p->normalize = (normalize_advantage && batch > 1) ? 1 : 0;
  p->device = v0->device; p->env_kind = v0->cfg.env_kind; p->ctbr = v0->cfg.wrapper == QUAD_WRAP_CTBR;
  p->spec = v0->spec; p->kc = v0->kdev;
  p->nb = lrn::layout_both(batch).nb;
  p->adam_nblocks = at[0].nblocks;
  p->fam_actor = arch != nullptr;
  p->fam_learner = fam_learner;
  p->deployed = deploy != nullptr;
  if (arch) p->arch = *arch;
  for (int32_t i = 0; i < P; i++) p->packed.push_back(members[i].packed);
  DeviceGuard g(p->device);
  hipError_t e = upload(&p->roll, roll.data(), roll.size() * sizeof(RollEntry));
  if (!e) e = upload(&p->gae, gae.data(), gae.size() * sizeof(GaeEntry));
  if (!e) e = upload(&p->pack, pack.data(), pack.size() * sizeof(PackEntry));
  if (!e) e = upload(&p->value, value.data(), value.size() * sizeof(ValueEntry));
  if (!e) e = upload(&p->lt.g, gt.data(), gt.size() * sizeof(lrn::GArgs));
  if (!e && !fam_learner) e = upload(&p->lt.r, rt.data(), rt.size() * sizeof(lrn::RArgs));
  if (!e && fam_learner) e = upload(&p->ga, ga.data(), ga.size() * sizeof(lrna::Args));
  if (!e && deploy) e = upload(&p->est, est.data(), est.size() * sizeof(EstEntry));
  if (!e) e = upload(&p->lt.a, at.data(), at.size() * sizeof(lrn::AdamArgs));
  if (e) {
    release(p);
    return hfail(fn.c_str(), e);
  }
  std::vector<int32_t> all(static_cast<size_t>(P));
  for (int32_t i = 0; i < P; i++) all[size_t(i)] = i;
  if (int rc = add_subset(p, all.data(), P, nullptr)) {  // subset 0: every member
    release(p);
    return rc;
  }
  *out = p;
  return QUAD_OK;
}

}  // namespace

extern "C" {

int64_t quad_pop_workspace_bytes(const QuadAdam* adam, int32_t batch) {
  if (batch < 1 || batch > POP_MAX_BATCH) return 0;
  return learner_workspace_bytes(adam, batch);
}

int64_t quad_pop_arch_workspace_bytes(const QuadActorArch* arch, const QuadAdam* adam, int32_t batch) {
  if (!lrna::in_family(arch) || batch < 1 || batch > POP_MAX_BATCH) return 0;
  const int64_t partials = adam_partials_bytes(adam);
  return partials ? arch_adam_offset(*arch, batch) + partials : 0;
}

int quad_pop_create(const QuadPopMember* members, int32_t P, int32_t batch, int32_t normalize_advantage,
                    QuadPop** out) {
  if (out) *out = nullptr;
  return create("quad_pop_create", nullptr, members, nullptr, P, batch, normalize_advantage, out);
}

int quad_pop_create_arch(const QuadActorArch* arch, const QuadPopMember* members, int32_t P, int32_t batch,
                         int32_t normalize_advantage, QuadPop** out) {
  if (out) *out = nullptr;
  if (!lrna::in_family(arch))
    return pfail("quad_pop_create_arch: the family is h1 a multiple of 32 in [32, 512], h2 in {64, 128, 256}, "
                 "QUAD_ACTFN_RELU or QUAD_ACTFN_TANH");
  return create("quad_pop_create_arch", arch, members, nullptr, P, batch, normalize_advantage, out);
}

int64_t quad_pop_deployed_workspace_bytes(const QuadActorArch* arch, const QuadAdam* adam, int32_t batch) {
  if (!lrna::in_family(arch)) return 0;
  return is_128_relu(*arch) ? quad_pop_workspace_bytes(adam, batch) : quad_pop_arch_workspace_bytes(arch, adam, batch);
}

int quad_pop_create_deployed(const QuadActorArch* arch, const QuadPopMember* members, const QuadPopDeploy* deploy,
                             int32_t P, int32_t batch, int32_t normalize_advantage, QuadPop** out) {
  if (out) *out = nullptr;
  if (!lrna::in_family(arch))
    return pfail("quad_pop_create_deployed: the family is h1 a multiple of 32 in [32, 512], h2 in {64, 128, 256}, "
                 "QUAD_ACTFN_RELU or QUAD_ACTFN_TANH");
  if (!deploy) return pfail("quad_pop_create_deployed: deploy is NULL");
  return create("quad_pop_create_deployed", arch, members, deploy, P, batch, normalize_advantage, out);
}

void quad_pop_destroy(QuadPop* pop) { release(pop); }

int quad_pop_subset(QuadPop* pop, const int32_t* members, int32_t count, int32_t* subset_id) {
  if (!pop || !subset_id) return pfail("quad_pop_subset: pop / subset_id is NULL");
  return add_subset(pop, members, count, subset_id);
}

int quad_pop_pack(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_pack");
  if (!s) return QUAD_EINVAL;
  DeviceGuard g(pop->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return pop->fam_actor ? launch_pop_ac_pack(pop->arch, pop->pack, s->dev, s->count, st)
                      : launch_pop_pack(pop->pack, s->dev, s->count, st);
}

int quad_pop_rollout(QuadPop* pop, int32_t subset, int32_t t0, int32_t steps, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_rollout");
  if (!s) return QUAD_EINVAL;
  if (steps < 1 || t0 < 0) return pfail("quad_pop_rollout: steps >= 1, t0 >= 0");
  DeviceGuard g(pop->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipError_t e = pop->deployed
                         ? launch_pop_ac_rollout_deployed(pop->arch, pop->kc, pop->roll, pop->est, s->dev, s->count,
                                                          pop->n, pop->env_kind, pop->ctbr, uint32_t(t0), steps, st)
                     : pop->fam_actor
                         ? launch_pop_ac_rollout(pop->arch, pop->kc, pop->roll, s->dev, s->count, pop->n, pop->env_kind,
                                                 pop->ctbr, uint32_t(t0), steps, st)
                         : launch_pop_rollout(pop->kc, pop->roll, s->dev, s->count, pop->n, pop->env_kind, pop->ctbr,
                                              pop->spec, uint32_t(t0), steps, st))
    return hfail("quad_pop_rollout", e);
  return QUAD_OK;
}

int quad_pop_value(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_value");
  if (!s) return QUAD_EINVAL;
  DeviceGuard g(pop->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return pop->fam_actor ? launch_pop_ac_value(pop->arch, pop->value, s->dev, s->count, pop->n, st)
                      : launch_pop_value(pop->value, s->dev, s->count, pop->n, st);
}

int quad_pop_gae(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_gae");
  if (!s) return QUAD_EINVAL;
  DeviceGuard g(pop->device);
  if (hipError_t e = launch_pop_gae(pop->gae, s->dev, s->count, pop->rows, pop->n, static_cast<hipStream_t>(stream)))
    return hfail("quad_pop_gae", e);
  return QUAD_OK;
}

int quad_pop_permutation(QuadPop* pop, int32_t subset, const uint64_t* seeds, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_permutation");
  if (!s) return QUAD_EINVAL;
  if (!seeds) return pfail("quad_pop_permutation: seeds is NULL");
  DeviceGuard g(pop->device);
  return launch_pop_permutation(pop->lt.g, s->dev, s->count, int64_t(pop->rows) * pop->n, seeds,
                                static_cast<hipStream_t>(stream));
}

int quad_pop_adv_stats_epoch(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_adv_stats_epoch");
  if (!s) return QUAD_EINVAL;
  if (!pop->normalize) return QUAD_OK;  // nothing reads the sums
  DeviceGuard g(pop->device);
  return launch_pop_adv_stats_epoch(pop->lt.g, s->dev, s->count, pop->nmb, static_cast<hipStream_t>(stream));
}

int quad_pop_ppo_grad(QuadPop* pop, int32_t subset, int32_t slot, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_ppo_grad");
  if (!s) return QUAD_EINVAL;
  if (slot < 0 || slot >= pop->nmb) return pfail("quad_pop_ppo_grad: slot out of range");
  DeviceGuard g(pop->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pop->fam_learner) return lrna::launch_pop_grad(pop->arch, pop->batch, pop->ga, s->dev, s->count, slot, st);
  if (int rc = lrn::launch_pop_grad_x3(pop->lt.g, s->dev, s->count, slot, pop->nb, st)) return rc;
  return launch_pop_reduce(pop->lt.r, s->dev, s->count, slot, st);
}

int quad_pop_clip_adam(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_clip_adam");
  if (!s) return QUAD_EINVAL;
  DeviceGuard g(pop->device);
  return launch_pop_clip_adam(pop->lt.a, s->dev, s->count, pop->adam_nblocks, static_cast<hipStream_t>(stream));
}

int quad_pop_attach_eval(QuadPop* pop, const QuadPopEval* evals) {
  if (!pop || !evals) return pfail("quad_pop_attach_eval: pop / evals is NULL");
  std::vector<PopEpisodeEntry> tab(static_cast<size_t>(pop->P));
  std::vector<char> ok(static_cast<size_t>(pop->P), 0);
  const QuadHandle* v0 = nullptr;
  int32_t first = -1;
  for (int32_t i = 0; i < pop->P; i++) {
    if (!evals[i].env) continue;  // a member that is not evaluated: no entry, quad_pop_episode rejects it
    const std::string who = "quad_pop_attach_eval: member " + std::to_string(i) + ": ";
    EpisodeArgs a{};
    if (int rc = episode_args(evals[i].env, pop->packed[size_t(i)], &evals[i].run, &a)) return rc;
    if (pop->deployed) {
      if (evals[i].run.obs_mode != QUAD_OBS_DEPLOYED)
        return pfail(who + "obs_mode must be QUAD_OBS_DEPLOYED on a quad_pop_create_deployed population");
    } else if (evals[i].run.obs_mode != QUAD_OBS_ENV) {
      return pfail(who + "obs_mode must be QUAD_OBS_ENV");
    }
    const QuadHandle* v = evals[i].env;
    if (first < 0) { first = i; v0 = v; }
    if (!same_envs(v, v0))
      return pfail(who + "env kind, wrapper, constants, env count or device differ from the first evaluated member's");
    if (evals[i].run.max_steps != evals[first].run.max_steps)
      return pfail(who + "max_steps differ from the first evaluated member's");
    if (v->device != pop->device) return pfail(who + "the evaluation handle is on another device");
    tab[size_t(i)] = PopEpisodeEntry{v->kp, pop->packed[size_t(i)], a};
    ok[size_t(i)] = 1;
  }
  if (first < 0) return pfail("quad_pop_attach_eval: no member has an evaluation handle");
  DeviceGuard g(pop->device);
  PopEpisodeEntry* dev = nullptr;
  if (hipError_t e = upload(&dev, tab.data(), tab.size() * sizeof(PopEpisodeEntry))) {
    (void)hipFree(dev);
    return hfail("quad_pop_attach_eval", e);
  }
  (void)hipFree(pop->eval);
  pop->eval = dev;
  pop->eval_ok = ok;
  pop->eval_kc = v0->kdev; pop->eval_n = v0->n; pop->eval_kind = v0->cfg.env_kind;
  pop->eval_ctbr = v0->cfg.wrapper == QUAD_WRAP_CTBR; pop->eval_spec = v0->spec;
  return QUAD_OK;
}

int quad_pop_detach_eval(QuadPop* pop) {
  if (!pop) return pfail("quad_pop_detach_eval: pop is NULL");
  DeviceGuard g(pop->device);
  (void)hipFree(pop->eval);  // (synchronizes: no launch still reads the table)
  pop->eval = nullptr;
  pop->eval_ok.clear();
  return QUAD_OK;
}

int quad_pop_episode(QuadPop* pop, int32_t subset, void* stream) {
  const QuadPop::Subset* s = subset_of(pop, subset, "quad_pop_episode");
  if (!s) return QUAD_EINVAL;
  if (!pop->eval) return pfail("quad_pop_episode: no evaluation table (quad_pop_attach_eval)");
  for (int32_t m : s->members)
    if (!pop->eval_ok[size_t(m)]) return pfail("quad_pop_episode: a member of the subset has no evaluation handle attached");
  DeviceGuard g(pop->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipError_t e = pop->fam_actor
                         ? launch_pop_actor_episode(pop->arch, pop->eval_kc, pop->eval, s->dev, s->count, pop->eval_n,
                                                    pop->eval_kind, pop->eval_ctbr,
                                                    pop->deployed ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV, st)
                         : launch_pop_policy_episode(pop->eval_kc, pop->eval, s->dev, s->count, pop->eval_n,
                                                     pop->eval_kind, pop->eval_ctbr, pop->eval_spec, st))
    return hfail("quad_pop_episode", e);
  return QUAD_OK;
}

}  // extern "C"
