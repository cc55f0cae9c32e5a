"""ctypes binding of libquadenv.so (the C ABI in include/quadenv.h).

The library is built in-tree by ``__graft_entry__.build()`` (``csrc/Makefile`` -> ``_lib/``).
There is no fallback: if the library is missing or fails to load, every env constructor raises.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "_lib", "libquadenv.so")
if os.environ.get("QUADENV_LIB"):  # A/B and ablation builds of the same library (tools/*_variants.sh)
    LIB_PATH = os.environ["QUADENV_LIB"]
CSRC = os.path.join(_PKG, "csrc")

QUAD_OK, QUAD_EINVAL, QUAD_EHIP, QUAD_ENOMEM, QUAD_EMODEL = 0, -1, -2, -3, -4
QUAD_ADV_PRECOMPUTED = 2  # QuadPPOBatch.normalize_advantage: quad_ppo_adv_stats already ran
QUAD_ADV_GIVEN = 3        # ... : the sums are in QuadPPOBatch.adv_sums (quad_ppo_adv_stats_epoch)
ADV_SUM_DOUBLES = 512     # QUAD_ADV_SUM_DOUBLES: one minibatch's block sums
ENV_HOVER, ENV_TRAJ, ENV_BRAX_HOVER, ENV_BRAX_TRAJ = 0, 1, 2, 3
WRAP_NONE, WRAP_CTBR, WRAP_RELPOS, WRAP_CTBR_RELPOS = 0, 1, 2, 3
ABI_VERSION = 8
PID_YAW_FRAME, PID_WORLD_FRAME = 0, 1
PID_RUNNING, PID_TERMINATED, PID_TRUNCATED, PID_INVALID = 0, 1, 2, 3
PID_LAP = 4  # quad_ctrl_waypoints / quad_policy_waypoints: the env completed its lap


class QuadCfg(C.Structure):
    _fields_ = [
        ("env_kind", C.c_int32), ("wrapper", C.c_int32), ("max_episode_steps", C.c_int32),
        ("auto_reset", C.c_int32),
        ("obs_low", C.c_float * 12), ("obs_high", C.c_float * 12),
        ("init_low", C.c_float * 12), ("init_high", C.c_float * 12),
        ("target_low", C.c_float * 3), ("target_high", C.c_float * 3),
        ("term_low", C.c_float * 12), ("term_high", C.c_float * 12),
        ("act_low", C.c_float * 4), ("act_high", C.c_float * 4),
        ("max_motor_thrust", C.c_double), ("arm_length", C.c_double), ("yaw_coeff", C.c_double),
        ("nominal_voltage", C.c_double), ("min_voltage", C.c_double),
        ("vdrop_base", C.c_double), ("vdrop_load", C.c_double),
        ("rate_max_rad", C.c_double), ("rate_kd", C.c_double * 3), ("rate_ki", C.c_double),
        ("rate_imax", C.c_double), ("inertia", C.c_double * 3), ("max_torque", C.c_double),
        ("timestep", C.c_double), ("gravity", C.c_double * 3), ("density", C.c_double),
        ("viscosity", C.c_double),
        ("reset_noise", C.c_float), ("reward_pos_coef", C.c_float),
        ("reward_action_coef", C.c_float), ("vel_limit", C.c_float),
        ("traj_center", C.c_float * 3), ("traj_amp", C.c_float * 3), ("traj_freq", C.c_float * 3),
        ("traj_duration", C.c_float),
        ("spline_center_low", C.c_float * 3), ("spline_center_high", C.c_float * 3),
        ("spline_amp", C.c_float * 3), ("spline_duration", C.c_float),
    ]


class QuadStateSoA(C.Structure):
    _fields_ = [("qpos", C.c_void_p), ("qvel", C.c_void_p), ("voltage", C.c_void_p),
                ("target", C.c_void_p), ("rate_int", C.c_void_p), ("step_count", C.c_void_p),
                ("episode", C.c_void_p), ("prev_action", C.c_void_p)]


class QuadStepOut(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p),
                ("truncated", C.c_void_p), ("terminal_obs", C.c_void_p),
                ("motor_commands", C.c_void_p), ("voltage_scale", C.c_void_p),
                ("state12", C.c_void_p), ("target_info", C.c_void_p)]


class QuadPolicyParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pi_w0", "pi_b0", "pi_w1", "pi_b1", "act_w", "act_b",
                                          "vf_w0", "vf_b0", "vf_w1", "vf_b1", "val_w", "val_b",
                                          "log_std")]


class QuadWaypoints(C.Structure):
    _fields_ = [("points", C.c_void_p), ("counts", C.c_void_p), ("set_of", C.c_void_p),
                ("max_points", C.c_int32), ("reach_radius", C.c_float)]


class QuadWaypointState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wp_idx", "reached", "laps", "steps", "status", "total_reward")]


class QuadWaypointRun(C.Structure):
    _fields_ = [("w", QuadWaypoints), ("s", QuadWaypointState), ("trace_reward", C.c_void_p),
                ("trace_wp_idx", C.c_void_p)]


# QuadPidGains: the 21 numbers of pid_gains.json in CascadedPIDController.__init__'s order, then MASS
PID_GAIN_FIELDS = ("kp_xy", "kd_xy", "ki_xy", "kp_z", "kd_z", "ki_z", "kp_att", "kd_att", "kp_yaw", "kd_yaw",
                   "ki_rate_torque", "rate_int_max", "axy_max", "az_min", "az_max", "tilt_max", "z_int_max",
                   "xy_int_max", "torque_motor_frac", "torque_abs_max", "yaw_torque_scale", "mass")


class QuadPidGains(C.Structure):
    _fields_ = [(n, C.c_double) for n in PID_GAIN_FIELDS]


# QuadPidMetrics: device [N] arrays; (name, torch dtype name)
PID_METRIC_FIELDS = (("steps", "int32"), ("status", "int32"), ("total_reward", "float64"),
                     ("pos_err_sum", "float64"), ("pos_err_sq", "float64"), ("pos_err_max", "float64"),
                     ("yaw_rate_abs_sum", "float64"), ("yaw_rate_sum", "float64"), ("yaw_rate_sq", "float64"),
                     ("yaw_rate_abs_max", "float64"), ("yaw_rate_sign_changes", "int32"),
                     ("yaw_rate_delta_sum", "float64"))


class QuadPidMetrics(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in PID_METRIC_FIELDS]


class QuadPidRun(C.Structure):
    _fields_ = [("gains", C.c_void_p), ("set_of", C.c_void_p), ("n_sets", C.c_int32), ("mode", C.c_int32),
                ("max_steps", C.c_int32), ("trace_envs", C.c_int32), ("integ", C.c_void_p),
                ("trace_actions", C.c_void_p), ("trace_state12", C.c_void_p), ("metrics", QuadPidMetrics)]


# the controller family: law ids (the PID ids equal the PID modes), QuadCtrlParams = QuadPidGains + extras
CTRL_PID_YAW, CTRL_PID_WORLD, CTRL_SE3, CTRL_SMC, CTRL_LQR = 0, 1, 2, 3, 4
CTRL_NSTATE, CTRL_NDIAG = 8, 7
CTRL_EXTRA_FIELDS = ("lqr_k0", "lqr_k1", "lqr_k2", "yaw_stw_k1", "yaw_stw_k2", "yaw_stw_boundary", "yaw_deadband",
                     "yaw_v_int_max", "yaw_rate_max", "yaw_rate_lpf_alpha", "se3_reorthonormalize")
CTRL_PARAM_FIELDS = PID_GAIN_FIELDS + CTRL_EXTRA_FIELDS


class QuadCtrlParams(C.Structure):
    _fields_ = [("base", QuadPidGains), ("lqr_k", C.c_double * 3)] + [(n, C.c_double) for n in CTRL_EXTRA_FIELDS[3:]]


class QuadCtrlRun(C.Structure):  # QuadPidRun's layout, field for field, under the family's names
    _fields_ = [({"gains": "params", "mode": "law", "integ": "state"}.get(n, n), t) for n, t in QuadPidRun._fields_]


# the deployed observation path (policy_node.py's estimator and builder) and the policy's fused episode
OBS_ENV, OBS_DEPLOYED = 0, 1
OBS_MODES = {"env": OBS_ENV, "deployed": OBS_DEPLOYED, OBS_ENV: OBS_ENV, OBS_DEPLOYED: OBS_DEPLOYED}
EST_NSTATE = 8


class QuadVelEst(C.Structure):
    _fields_ = [("alpha", C.c_void_p), ("alpha_all", C.c_double), ("max_dt", C.c_double), ("state", C.c_void_p)]


class QuadPolicyRun(C.Structure):
    _fields_ = [("obs_mode", C.c_int32), ("max_steps", C.c_int32), ("trace_envs", C.c_int32),
                ("est", QuadVelEst), ("est_dt", C.c_double),
                ("trace_actions", C.c_void_p), ("trace_state12", C.c_void_p), ("trace_obs", C.c_void_p),
                ("trace_vel_est", C.c_void_p), ("metrics", QuadPidMetrics), ("vel_err_sq", C.c_void_p)]


# the general actor (quad_actor_*): 12 -> h1 -> h2 -> 4, h1 a multiple of 32 up to 512, h2 in ACTOR_H2
ACTFN_RELU, ACTFN_TANH = 0, 1
ACTFNS = {"relu": ACTFN_RELU, "tanh": ACTFN_TANH}
ACTOR_MAX_H1, ACTOR_H2 = 512, (64, 128, 256)


class QuadActorArch(C.Structure):
    _fields_ = [("h1", C.c_int32), ("h2", C.c_int32), ("activation", C.c_int32)]


class QuadActorParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w0", "b0", "w1", "b1", "w2", "b2")]


# the Brax-profile policy (quad_brax_*): 21 -> h1 -> h2 -> 8 behind the running statistics' normaliser; the general
# actor's widths, and SiLU beside ReLU and tanh
ACTFN_SILU = 2
BRAX_ACTFNS = {"relu": ACTFN_RELU, "tanh": ACTFN_TANH, "silu": ACTFN_SILU}
BRAX_OBS, BRAX_LOGITS = 21, 8


class QuadBraxActorArch(C.Structure):
    _fields_ = [("h1", C.c_int32), ("h2", C.c_int32), ("activation", C.c_int32)]


class QuadBraxActorParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w0", "b0", "w1", "b1", "w2", "b2", "mean", "std")] + \
               [("min_std", C.c_float)]


# QuadBraxMetrics: device [N] arrays; (name, torch dtype name)
BRAX_METRIC_FIELDS = (("ret", "float64"), ("steps", "int32"), ("err_sum", "float64"), ("err_sq_sum", "float64"),
                      ("err_count", "int32"), ("status", "int32"))


class QuadBraxMetrics(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in BRAX_METRIC_FIELDS]


class QuadBraxRun(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("trace_envs", C.c_int32), ("deterministic", C.c_int32),
                ("noise_step0", C.c_uint32), ("seed", C.c_uint64), ("metrics", QuadBraxMetrics),
                ("trace_actions", C.c_void_p), ("trace_obs", C.c_void_p), ("trace_pos", C.c_void_p),
                ("trace_target", C.c_void_p)]


class QuadBraxPPOParams(C.Structure):
    """quad_brax_ppo_grad's nets: flax [in, out] kernels and biases, the normaliser, the checked arch."""
    _fields_ = [(n, C.c_void_p) for n in ("pi_w0", "pi_b0", "pi_w1", "pi_b1", "pi_w2", "pi_b2",
                                          "vf_w0", "vf_b0", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "mean", "std")] + \
               [("min_std", C.c_float)] + \
               [(n, C.c_int32) for n in ("policy_h1", "policy_h2", "value_h1", "value_h2", "activation")]


class QuadBraxPPOGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pi_w0", "pi_b0", "pi_w1", "pi_b1", "pi_w2", "pi_b2",
                                          "vf_w0", "vf_b0", "vf_w1", "vf_b1", "vf_w2", "vf_b2")]


class QuadBraxPPOBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "next_obs", "raw", "log_prob", "reward", "discount", "truncation",
                                          "index", "entropy_noise", "noise_out", "values", "vs", "advantages",
                                          "stats")] + \
               [(n, C.c_int32) for n in ("U", "L", "N", "mb")] + \
               [(n, C.c_float) for n in ("clipping_epsilon", "entropy_cost", "discounting", "gae_lambda",
                                         "reward_scaling")] + \
               [("normalize_advantage", C.c_int32), ("noise_step", C.c_uint32), ("seed", C.c_uint64)]


BRAX_PPO_HIDDEN, BRAX_PPO_MAX_L = (128, 128), 64  # quad_brax_ppo_grad's family
# quad_brax_ppo_arch_grad's family: each net's (h1, h2) with h1 a multiple of 32 in [32, BRAX_PPO_ARCH_MAX_H1] and h2
# in BRAX_PPO_ARCH_H2, any of BRAX_ACTFNS, unroll_length in [1, BRAX_PPO_MAX_L], at most BRAX_PPO_ARCH_MAX_ROWS loss rows
BRAX_PPO_ARCH_MAX_H1, BRAX_PPO_ARCH_H2, BRAX_PPO_ARCH_MAX_ROWS = 512, (64, 128, 256), 1 << 22

POLICY_STAT_SLOTS = 1024


class QuadBraxUnroll(C.Structure):
    """quad_brax_unroll's descriptor: time-major row buffers [steps, N, .], next_obs [steps / unroll_length, N, 21],
    ep_ret [N], stats [POLICY_STAT_SLOTS, 2] float64 (return sum, episodes)."""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "raw", "log_prob", "reward", "discount", "truncation", "next_obs",
                                          "ep_ret", "stats")] + \
               [("steps", C.c_int32), ("unroll_length", C.c_int32), ("noise_step0", C.c_uint32),
                ("seed", C.c_uint64)]


class QuadRolloutPost(C.Structure):
    _fields_ = [("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p),
                ("terminal_obs", C.c_void_p), ("buf_rew", C.c_void_p), ("last_start", C.c_void_p),
                ("ep_ret", C.c_void_p), ("ep_len", C.c_void_p), ("stats", C.c_void_p),
                ("rows", C.c_int32), ("gamma", C.c_float)]


class QuadPolicyAct(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("actions_env", C.c_void_p), ("actions", C.c_void_p),
                ("log_prob", C.c_void_p), ("value", C.c_void_p), ("obs_copy", C.c_void_p),
                ("last_start", C.c_void_p), ("episode_starts", C.c_void_p),
                ("cursor", C.c_void_p), ("rows", C.c_int32), ("deterministic", C.c_int32),
                ("seed", C.c_uint64), ("env_id_base", C.c_uint64),
                ("epilogue", C.POINTER(QuadRolloutPost))]


# every symbol include/quadenv.h declares (checked by tests/test_abi.py)
EXPORTS = ("quad_abi_version", "quad_last_error", "quad_default_cfg", "quad_create",
           "quad_destroy", "quad_num_envs", "quad_seed", "quad_reset", "quad_step", "quad_step_range", "quad_observe", "quad_terminated", "quad_step_random",
           "quad_mem_floor",
           "quad_kernel_form", "quad_random_actions", "quad_get_state", "quad_set_state", "quad_gae",
           "quad_policy_packed_floats", "quad_policy_pack", "quad_policy_act", "quad_rollout_post", "quad_rollout",
           "quad_waypoints_begin", "quad_waypoints_update", "quad_ppo_workspace_bytes", "quad_ppo_grad",
           "quad_ppo_grad_form", "quad_ppo_hidden", "quad_ppo_adv_stats", "quad_ppo_adv_stats_epoch", "quad_permutation", "quad_adam_workspace_bytes",
           "quad_clip_adam",
           "quad_pid_default_gains", "quad_pid_act", "quad_pid_episode", "quad_target_info",
           "quad_ctrl_default_params", "quad_ctrl_act", "quad_ctrl_episode",
           "quad_deploy_obs", "quad_policy_episode", "quad_ctrl_waypoints", "quad_policy_waypoints",
           "quad_actor_packed_floats", "quad_actor_pack", "quad_actor_act", "quad_actor_episode",
           "quad_actor_waypoints",
           "quad_brax_actor_packed_floats", "quad_brax_actor_pack", "quad_brax_actor_act", "quad_brax_episode",
           "quad_brax_actor_sample", "quad_brax_unroll", "quad_brax_ppo_workspace_bytes", "quad_brax_ppo_grad",
           "quad_brax_ppo_arch_workspace_bytes", "quad_brax_ppo_arch_grad",
           "quad_ppo_arch_workspace_bytes", "quad_ppo_arch_grad",
           "quad_actor_critic_packed_floats", "quad_actor_critic_pack", "quad_actor_critic_act",
           "quad_actor_critic_post", "quad_actor_rollout",
           "quad_deploy_obs_rows", "quad_actor_rollout_deployed")


class QuadRollout(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs_copy", "actions", "log_prob", "value", "episode_starts",
                                          "rewards", "last_obs", "last_start", "ep_ret", "ep_len",
                                          "stats")] + \
               [("rows", C.c_int32), ("t0", C.c_int32), ("steps", C.c_int32), ("deterministic", C.c_int32),
                ("seed", C.c_uint64), ("gamma", C.c_float)]


class QuadPolicyGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pi_w0", "pi_b0", "pi_w1", "pi_b1", "act_w", "act_b",
                                          "vf_w0", "vf_b0", "vf_w1", "vf_b1", "val_w", "val_b",
                                          "log_std")]


class QuadPPOBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "log_prob", "advantages", "returns", "index")] + \
               [("batch", C.c_int32), ("normalize_advantage", C.c_int32), ("clip_range", C.c_float),
                ("ent_coef", C.c_float), ("vf_coef", C.c_float), ("stats", C.c_void_p), ("adv_sums", C.c_void_p)]


ADAM_MAX_TENSORS = 16


class QuadAdam(C.Structure):
    _fields_ = [(n, C.c_void_p * ADAM_MAX_TENSORS) for n in ("params", "grads", "exp_avg", "exp_avg_sq", "step")] + \
               [("numel", C.c_int32 * ADAM_MAX_TENSORS), ("count", C.c_int32), ("max_grad_norm", C.c_float),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


POP_MAX_BATCH = 8192  # quad_pop_create: the separate-block gradient form's minibatch limit


class QuadPopMember(C.Structure):
    """One member of a lock-step PPO population (quad_pop_create; include/quadenv.h)."""
    _fields_ = [("env", C.c_void_p), ("params", QuadPolicyParams), ("grads", QuadPolicyGrads), ("adam", QuadAdam),
                ("packed", C.c_void_p), ("rollout", QuadRollout), ("last_values", C.c_void_p),
                ("scratch_actions", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
                ("perm", C.c_void_p), ("adv_sums", C.c_void_p), ("mb_stats", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("gae_lambda", C.c_float), ("clip_range", C.c_float), ("ent_coef", C.c_float), ("vf_coef", C.c_float)]


class QuadPopEval(C.Structure):
    _fields_ = [("env", C.c_void_p), ("run", QuadPolicyRun)]


POP_EXPORTS = ("quad_pop_workspace_bytes", "quad_pop_create", "quad_pop_destroy", "quad_pop_subset", "quad_pop_pack",
               "quad_pop_rollout", "quad_pop_value", "quad_pop_gae", "quad_pop_permutation",
               "quad_pop_adv_stats_epoch", "quad_pop_ppo_grad", "quad_pop_clip_adam", "quad_pop_attach_eval",
               "quad_pop_detach_eval", "quad_pop_episode")
# the general family's populations: the same launch calls on a QuadPop of quad_pop_create_arch
POP_ARCH_EXPORTS = ("quad_pop_arch_workspace_bytes", "quad_pop_create_arch")


class QuadPopDeploy(C.Structure):
    """One member's estimator in a population trained on the deployed observation (quad_pop_create_deployed)."""
    _fields_ = [("est", QuadVelEst), ("est_dt", C.c_double)]


# populations on the deployed observation: the same launch calls on a QuadPop of quad_pop_create_deployed
POP_DEPLOYED_EXPORTS = ("quad_pop_deployed_workspace_bytes", "quad_pop_create_deployed")
EXPORTS = EXPORTS + POP_EXPORTS + POP_ARCH_EXPORTS + POP_DEPLOYED_EXPORTS


class QuadError(RuntimeError):
    pass


_lib = None


def _declare(L):
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    L.quad_abi_version.restype = C.c_int
    L.quad_last_error.restype = C.c_char_p
    L.quad_default_cfg.argtypes = [i32, i32, C.POINTER(QuadCfg)]
    L.quad_create.argtypes = [C.POINTER(QuadCfg), i32, u64, u64, i32, C.POINTER(vp)]
    L.quad_destroy.argtypes = [vp]
    L.quad_destroy.restype = None
    L.quad_num_envs.argtypes = [vp]
    L.quad_num_envs.restype = i32
    L.quad_seed.argtypes = [vp, u64, vp]
    L.quad_reset.argtypes = [vp, vp, vp, vp]
    L.quad_step.argtypes = [vp, vp, C.POINTER(QuadStepOut), vp]
    L.quad_step_range.argtypes = [vp, i32, i32, vp, C.POINTER(QuadStepOut), vp]
    L.quad_observe.argtypes = [vp, vp, vp, vp]
    L.quad_terminated.argtypes = [vp, vp, i32, vp, vp]
    L.quad_step_random.argtypes = [vp, u32, i32, C.POINTER(QuadStepOut), vp, vp]
    if hasattr(L, "quad_mem_floor"):  # (added in round 6 as a backward-compatible entry; A/B tools load older builds)
        L.quad_mem_floor.argtypes = [vp, vp, C.POINTER(QuadStepOut), vp]
    L.quad_kernel_form.argtypes = [vp]
    L.quad_kernel_form.restype = i32
    L.quad_random_actions.argtypes = [vp, u32, vp, vp]
    L.quad_get_state.argtypes = [vp, C.POINTER(QuadStateSoA), i32, vp]
    L.quad_set_state.argtypes = [vp, C.POINTER(QuadStateSoA), i32, vp]
    L.quad_gae.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp, vp, vp]
    L.quad_policy_packed_floats.argtypes = []
    L.quad_policy_packed_floats.restype = i32
    L.quad_policy_pack.argtypes = [C.POINTER(QuadPolicyParams), vp, vp]
    L.quad_policy_act.argtypes = [vp, C.POINTER(QuadPolicyAct), i32, vp]
    L.quad_rollout_post.argtypes = [vp, C.POINTER(QuadRolloutPost), vp, i32, vp]
    L.quad_rollout.argtypes = [vp, vp, C.POINTER(QuadRollout), vp]
    L.quad_waypoints_begin.argtypes = [vp, C.POINTER(QuadWaypoints), C.POINTER(QuadWaypointState), vp, vp]
    L.quad_waypoints_update.argtypes = [vp, C.POINTER(QuadWaypoints), C.POINTER(QuadWaypointState),
                                        vp, vp, vp, vp, vp]
    L.quad_ppo_workspace_bytes.argtypes = [i32]
    L.quad_ppo_workspace_bytes.restype = C.c_int64
    L.quad_ppo_grad_form.argtypes = []
    L.quad_ppo_grad_form.restype = i32
    L.quad_permutation.argtypes = [C.c_int64, u64, vp, vp]
    L.quad_ppo_grad.argtypes = [C.POINTER(QuadPolicyParams), C.POINTER(QuadPPOBatch), C.POINTER(QuadPolicyGrads),
                                vp, C.c_int64, vp]
    L.quad_ppo_hidden.argtypes = [C.POINTER(QuadPolicyParams), C.POINTER(QuadPPOBatch), C.POINTER(QuadPolicyGrads),
                                  vp, vp, C.c_int64, vp]
    L.quad_ppo_adv_stats.argtypes = [C.POINTER(QuadPPOBatch), vp, C.c_int64, vp]
    L.quad_ppo_adv_stats_epoch.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.quad_adam_workspace_bytes.argtypes = [C.POINTER(QuadAdam)]
    L.quad_adam_workspace_bytes.restype = C.c_int64
    L.quad_clip_adam.argtypes = [C.POINTER(QuadAdam), vp, C.c_int64, vp]
    L.quad_pid_default_gains.argtypes = [C.POINTER(QuadPidGains)]
    L.quad_pid_act.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    L.quad_pid_episode.argtypes = [vp, C.POINTER(QuadPidRun), vp]
    L.quad_target_info.argtypes = [vp, vp, vp]
    L.quad_ctrl_default_params.argtypes = [C.POINTER(QuadCtrlParams)]
    L.quad_ctrl_act.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    L.quad_ctrl_episode.argtypes = [vp, C.POINTER(QuadCtrlRun), vp]
    L.quad_deploy_obs.argtypes = [vp, C.POINTER(QuadVelEst), vp, vp, C.c_double, i32, vp, vp, vp]
    L.quad_policy_episode.argtypes = [vp, vp, C.POINTER(QuadPolicyRun), vp]
    L.quad_ctrl_waypoints.argtypes = [vp, C.POINTER(QuadCtrlRun), C.POINTER(QuadWaypointRun), vp]
    L.quad_policy_waypoints.argtypes = [vp, vp, C.POINTER(QuadPolicyRun), C.POINTER(QuadWaypointRun), vp]
    if not hasattr(L, "quad_actor_act"):  # the version number did not change with the quad_actor_* additions
        raise QuadError(f"{LIB_PATH} was built before the general actor's entry points (quad_actor_*); rebuild it")
    arch = C.POINTER(QuadActorArch)
    L.quad_actor_packed_floats.argtypes = [arch]
    L.quad_actor_packed_floats.restype = C.c_int64
    L.quad_actor_pack.argtypes = [arch, C.POINTER(QuadActorParams), vp, vp]
    L.quad_actor_act.argtypes = [arch, vp, vp, vp, vp, i32, vp]
    L.quad_actor_episode.argtypes = [vp, arch, vp, C.POINTER(QuadPolicyRun), vp]
    L.quad_actor_waypoints.argtypes = [vp, arch, vp, C.POINTER(QuadPolicyRun), C.POINTER(QuadWaypointRun), vp]
    for n in ("quad_actor_pack", "quad_actor_act", "quad_actor_episode", "quad_actor_waypoints"):
        getattr(L, n).restype = C.c_int
    if not hasattr(L, "quad_brax_episode"):  # the version number did not change with the quad_brax_* additions
        raise QuadError(f"{LIB_PATH} was built before the Brax policy's entry points (quad_brax_*); rebuild it")
    barch = C.POINTER(QuadBraxActorArch)
    L.quad_brax_actor_packed_floats.argtypes = [barch]
    L.quad_brax_actor_packed_floats.restype = C.c_int64
    L.quad_brax_actor_pack.argtypes = [barch, C.POINTER(QuadBraxActorParams), vp, vp]
    L.quad_brax_actor_act.argtypes = [barch, vp, vp, vp, vp, i32, i32, u64, u64, u32, vp]
    L.quad_brax_episode.argtypes = [vp, barch, vp, C.POINTER(QuadBraxRun), vp]
    for n in ("quad_brax_actor_pack", "quad_brax_actor_act", "quad_brax_episode"):
        getattr(L, n).restype = C.c_int
    if not hasattr(L, "quad_brax_unroll"):  # nor with the learner's unroll entry points
        raise QuadError(f"{LIB_PATH} was built before the Brax unroll's entry points (quad_brax_unroll); rebuild it")
    L.quad_brax_actor_sample.argtypes = [barch, vp, vp, vp, vp, vp, vp, i32, u64, u64, u32, vp]
    L.quad_brax_unroll.argtypes = [vp, barch, vp, C.POINTER(QuadBraxUnroll), vp]
    for n in ("quad_brax_actor_sample", "quad_brax_unroll"):
        getattr(L, n).restype = C.c_int
    if not hasattr(L, "quad_brax_ppo_grad"):  # nor with the learner's gradient entry points
        raise QuadError(f"{LIB_PATH} was built before the Brax gradient's entry points (quad_brax_ppo_grad); rebuild it")
    L.quad_brax_ppo_workspace_bytes.argtypes = [i32, i32]
    L.quad_brax_ppo_workspace_bytes.restype = C.c_int64
    L.quad_brax_ppo_grad.argtypes = [C.POINTER(QuadBraxPPOParams), C.POINTER(QuadBraxPPOBatch),
                                     C.POINTER(QuadBraxPPOGrads), vp, C.c_int64, vp]
    L.quad_brax_ppo_grad.restype = C.c_int
    if not hasattr(L, "quad_brax_ppo_arch_grad"):  # nor with the whole family's gradient
        raise QuadError(f"{LIB_PATH} was built before the Brax family's gradient (quad_brax_ppo_arch_grad); rebuild it")
    L.quad_brax_ppo_arch_workspace_bytes.argtypes = [C.POINTER(QuadBraxPPOParams), i32, i32]
    L.quad_brax_ppo_arch_workspace_bytes.restype = C.c_int64
    L.quad_brax_ppo_arch_grad.argtypes = L.quad_brax_ppo_grad.argtypes
    L.quad_brax_ppo_arch_grad.restype = C.c_int
    if not hasattr(L, "quad_ppo_arch_grad"):  # nor with the general learner's
        raise QuadError(f"{LIB_PATH} was built before the general learner's entry points (quad_ppo_arch_grad); rebuild it")
    L.quad_ppo_arch_workspace_bytes.argtypes = [arch, i32]
    L.quad_ppo_arch_workspace_bytes.restype = C.c_int64
    L.quad_ppo_arch_grad.argtypes = [arch, C.POINTER(QuadPolicyParams), C.POINTER(QuadPPOBatch),
                                     C.POINTER(QuadPolicyGrads), vp, C.c_int64, vp]
    L.quad_ppo_arch_grad.restype = C.c_int
    if not hasattr(L, "quad_actor_rollout"):  # nor with the general family's rollout
        raise QuadError(f"{LIB_PATH} was built before the general rollout's entry points (quad_actor_rollout); rebuild it")
    L.quad_actor_critic_packed_floats.argtypes = [arch]
    L.quad_actor_critic_packed_floats.restype = C.c_int64
    L.quad_actor_critic_pack.argtypes = [arch, C.POINTER(QuadPolicyParams), vp, vp]
    L.quad_actor_critic_act.argtypes = [arch, vp, C.POINTER(QuadPolicyAct), i32, vp]
    L.quad_actor_critic_post.argtypes = [arch, vp, C.POINTER(QuadRolloutPost), vp, i32, vp]
    L.quad_actor_rollout.argtypes = [vp, arch, vp, C.POINTER(QuadRollout), vp]
    for n in ("quad_actor_critic_pack", "quad_actor_critic_act", "quad_actor_critic_post", "quad_actor_rollout"):
        getattr(L, n).restype = C.c_int
    # the deployed-observation rollout. A library built before it still loads (the A/B tools time such
    # builds against this tree); need_deployed() is what the callers of the two entry points ask first
    if hasattr(L, "quad_actor_rollout_deployed"):
        L.quad_deploy_obs_rows.argtypes = [vp, C.POINTER(QuadVelEst), vp, vp, vp, vp, i32, vp, vp, vp]
        L.quad_actor_rollout_deployed.argtypes = [vp, arch, vp, C.POINTER(QuadRollout), C.POINTER(QuadVelEst),
                                                  C.c_double, vp]
        for n in ("quad_deploy_obs_rows", "quad_actor_rollout_deployed"):
            getattr(L, n).restype = C.c_int
    if not hasattr(L, "quad_pop_create"):  # the version number did not change with the quad_pop_* additions
        raise QuadError(f"{LIB_PATH} was built before the population entry points (quad_pop_*); rebuild it")
    L.quad_pop_detach_eval.argtypes = [vp]
    L.quad_pop_workspace_bytes.argtypes = [C.POINTER(QuadAdam), i32]
    L.quad_pop_workspace_bytes.restype = C.c_int64
    L.quad_pop_create.argtypes = [C.POINTER(QuadPopMember), i32, i32, i32, C.POINTER(vp)]
    L.quad_pop_destroy.argtypes = [vp]
    L.quad_pop_destroy.restype = None
    L.quad_pop_subset.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32)]
    L.quad_pop_rollout.argtypes = [vp, i32, i32, i32, vp]
    L.quad_pop_permutation.argtypes = [vp, i32, vp, vp]
    L.quad_pop_ppo_grad.argtypes = [vp, i32, i32, vp]
    L.quad_pop_attach_eval.argtypes = [vp, C.POINTER(QuadPopEval)]
    for n in ("quad_pop_pack", "quad_pop_value", "quad_pop_gae", "quad_pop_adv_stats_epoch", "quad_pop_clip_adam",
              "quad_pop_episode"):
        getattr(L, n).argtypes = [vp, i32, vp]
    for n in POP_EXPORTS[1:]:
        if n != "quad_pop_destroy":
            getattr(L, n).restype = C.c_int
    if not hasattr(L, "quad_pop_create_arch"):  # nor with the general family's populations
        raise QuadError(f"{LIB_PATH} was built before the general family's populations (quad_pop_create_arch); "
                        "rebuild it")
    L.quad_pop_arch_workspace_bytes.argtypes = [arch, C.POINTER(QuadAdam), i32]
    L.quad_pop_arch_workspace_bytes.restype = C.c_int64
    L.quad_pop_create_arch.argtypes = [arch, C.POINTER(QuadPopMember), i32, i32, i32, C.POINTER(vp)]
    L.quad_pop_create_arch.restype = C.c_int
    # populations on the deployed observation. As with the deployed rollout, a library built before them
    # still loads; need_deployed_population() is what their callers ask first
    if hasattr(L, "quad_pop_create_deployed"):
        L.quad_pop_deployed_workspace_bytes.argtypes = [arch, C.POINTER(QuadAdam), i32]
        L.quad_pop_deployed_workspace_bytes.restype = C.c_int64
        L.quad_pop_create_deployed.argtypes = [arch, C.POINTER(QuadPopMember), C.POINTER(QuadPopDeploy), i32, i32, i32,
                                               C.POINTER(vp)]
        L.quad_pop_create_deployed.restype = C.c_int
    for n in ("quad_pid_default_gains", "quad_pid_act", "quad_pid_episode", "quad_target_info",
              "quad_ctrl_default_params", "quad_ctrl_act", "quad_ctrl_episode", "quad_deploy_obs",
              "quad_policy_episode", "quad_ctrl_waypoints", "quad_policy_waypoints"):
        getattr(L, n).restype = C.c_int
    for n in ("quad_clip_adam", "quad_ppo_grad", "quad_ppo_hidden", "quad_ppo_adv_stats", "quad_ppo_adv_stats_epoch", "quad_default_cfg", "quad_create", "quad_seed", "quad_reset", "quad_step", "quad_step_range", "quad_observe", "quad_terminated", "quad_step_random",
              "quad_random_actions", "quad_get_state", "quad_set_state", "quad_gae",
              "quad_policy_pack", "quad_policy_act", "quad_rollout_post", "quad_rollout",
              "quad_waypoints_begin", "quad_waypoints_update"):
        getattr(L, n).restype = C.c_int


def lib():
    """Load libquadenv.so; raise loudly if it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QuadError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                            f"g.build()'` (or make -C {CSRC}) to build the HIP extension")
        L = C.CDLL(LIB_PATH)
        _declare(L)
        if L.quad_abi_version() != ABI_VERSION:
            raise QuadError("libquadenv.so ABI version mismatch; rebuild it")
        _lib = L
    return _lib


def need_deployed():
    """lib(), or QuadError when it was built before quad_deploy_obs_rows / quad_actor_rollout_deployed."""
    L = lib()
    if not hasattr(L, "quad_actor_rollout_deployed"):
        raise QuadError(f"{LIB_PATH} was built before the deployed rollout's entry points "
                        "(quad_actor_rollout_deployed); rebuild it")
    return L


def need_deployed_population():
    """need_deployed(), or QuadError when the library was built before quad_pop_create_deployed."""
    L = need_deployed()
    if not hasattr(L, "quad_pop_create_deployed"):
        raise QuadError(f"{LIB_PATH} was built before the deployed populations' entry points "
                        "(quad_pop_create_deployed); rebuild it")
    return L


def check(rc: int, what: str = "") -> None:
    if rc != QUAD_OK:
        msg = lib().quad_last_error().decode(errors="replace")
        raise QuadError(f"{what} failed ({rc}): {msg}")


def default_cfg(env_kind: int = ENV_HOVER, wrapper: int = WRAP_NONE) -> QuadCfg:
    cfg = QuadCfg()
    check(lib().quad_default_cfg(env_kind, wrapper, C.byref(cfg)), "quad_default_cfg")
    return cfg
