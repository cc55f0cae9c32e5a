/*
 * quadenv.h -- C ABI of libquadenv.so, the MI355X-native vectorized quadrotor env.
 *
 * This is the drop-in boundary for the reference's hot path: N independent copies of
 *   HoverEnv.step / HoverEnv.reset                 (envs/hover_env.py:159-198, :200-238)
 *   RateControlWrapper.action / .step / .reset      (envs/rate_wrapper.py:69-111)
 *   TrajectoryFollowEnv.step / .reset               (envs/trajectory_follow_env.py:145-174,
 *                                                    :220-253)
 * including the mujoco.mj_step they call (hover_env.py:180) and the SB3 VecEnv auto-reset
 * around them (train.py:48, DummyVecEnv semantics), executed as HIP kernels on gfx950 over a
 * struct-of-arrays batch resident in HBM.
 *
 * Conventions
 *  - Plain C types only; `void* stream` is a hipStream_t (e.g. torch.cuda.current_stream()
 *    .cuda_stream); NULL = the legacy default stream. Every call that launches work enqueues it
 *    on that stream and returns without synchronizing (graph-capturable), except get/set_state
 *    with host pointers, which synchronize the stream.
 *  - Device pointers are caller-owned (torch tensors' data_ptr()); the handle owns only the env
 *    state. Row-major shapes are given as [rows, cols].
 *  - Return 0 on success, a negative QUAD_E* code on error; the message is available from
 *    quad_last_error() (thread-local). Nothing aborts or throws across the ABI.
 *  - A handle is bound to one device and is not internally locked (one handle per process per
 *    GPU; multi-GPU = one process per GPU with disjoint env_id_base ranges).
 */
#ifndef QUADENV_H
#define QUADENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QUADENV_ABI_VERSION 8

enum { QUAD_OK = 0, QUAD_EINVAL = -1, QUAD_EHIP = -2, QUAD_ENOMEM = -3, QUAD_EMODEL = -4 };
/* QUAD_ENV_BRAX_HOVER / QUAD_ENV_BRAX_TRAJ: the brax Env API siblings of the same path
 * (train_brax_ppo.py QuadHoverBraxEnv :39-176 / JaxMJXQuadBraxEnv :179-368) as brax's ppo.train
 * wraps them (EpisodeWrapper truncation, AutoResetWrapper restoring the episode's first state):
 * 21-D raw obs [qpos(11), qvel(10)], clipped physical action -> mixer (no voltage), mjx.step
 * semantics (no MuJoCo-C bad-state resets). */
enum { QUAD_ENV_HOVER = 0, QUAD_ENV_TRAJ = 1, QUAD_ENV_BRAX_HOVER = 2, QUAD_ENV_BRAX_TRAJ = 3 };
/* QUAD_WRAP_RELPOS: RelPosActWrapper (envs/wrappers.py:13-25): 7-D obs [normalized rel pos (3),
 * previous action (4)] of the hover / trajectory kinds (quad_step's obs is then [N,7]).
 * QUAD_WRAP_CTBR_RELPOS: the stack the reference README documents,
 * RelPosActWrapper(RateControlWrapper(env)): the CTBR controller maps the rate action to torques
 * (rate_wrapper.py:69-98) and the 7-D obs carries the RATE action as the previous action
 * (rate_wrapper.py:100-106 overwrites unwrapped._prev_action after the base step). */
enum { QUAD_WRAP_NONE = 0, QUAD_WRAP_CTBR = 1, QUAD_WRAP_RELPOS = 2, QUAD_WRAP_CTBR_RELPOS = 3 };
enum { QUAD_NQ = 11, QUAD_NV = 10, QUAD_OBS = 12, QUAD_OBS_BRAX = 21, QUAD_OBS_RELPOS = 7, QUAD_ACT = 4 };

/* Env configuration. quad_default_cfg() fills the reference's defaults:
 *  HoverEnv.__init__ (hover_env.py:15-100), TrajectoryFollowEnv.__init__
 *  (trajectory_follow_env.py:22-104), RateControlWrapper.__init__ (rate_wrapper.py:40-64) with
 *  pid_gains.json:43-52, drone_config.py:9-22, drone.xml:4 (timestep, gravity, fluid). */
typedef struct QuadCfg {
  int32_t env_kind;          /* QUAD_ENV_HOVER | QUAD_ENV_TRAJ */
  int32_t wrapper;           /* QUAD_WRAP_NONE | _CTBR (RateControlWrapper) | _RELPOS | _CTBR_RELPOS */
  int32_t max_episode_steps; /* 512 hover / 2048 traj */
  int32_t auto_reset;        /* 1: SB3 VecEnv semantics (reset on terminated|truncated) */
  float obs_low[12], obs_high[12];       /* HoverEnv._obs_bounds   (normalization) */
  float init_low[12], init_high[12];     /* HoverEnv._initial_state_bounds */
  float target_low[3], target_high[3];   /* HoverEnv._target_pos_bounds (hover only) */
  float term_low[12], term_high[12];     /* HoverEnv._state_bounds (termination) */
  float act_low[4], act_high[4];         /* HoverEnv._action_bounds */
  double max_motor_thrust, arm_length, yaw_coeff; /* max_motor_thrust: finite, >= 0 (else QUAD_EINVAL) */
  double nominal_voltage, min_voltage, vdrop_base, vdrop_load;
  double rate_max_rad, rate_kd[3], rate_ki, rate_imax, inertia[3], max_torque;
  double timestep, gravity[3], density, viscosity;
  /* brax kinds only (train_brax_ppo.py): target = target_low (QuadHoverBraxEnv (0,0,1));
   * position limits = term_low/high[0..2] (|x|,|y| <= 3, z in [0.02, 4]); act_low/high = the
   * clip range of the physical action; max_episode_steps = --episode-length (500). */
  float reset_noise;            /* U(+-noise) on qpos and qvel at reset (0.01) */
  float reward_pos_coef;        /* exp(-coef |pos - target|^2): 2 hover, 1 jax_mjx */
  float reward_action_coef;     /* - coef |a|^2 (jax_mjx 0.001) */
  float vel_limit;              /* jax_mjx: any |v_i| > limit invalidates (20) */
  float traj_center[3], traj_amp[3], traj_freq[3];  /* jax_mjx sinusoid target */
  float traj_duration;          /* seconds spanned by the episode_length samples (5) */
  /* TrajectoryFollowEnv's info-only spline (trajectory_follow_env.py:175-243): center ~
   * U(spline_center_low, _high), n_wp ~ {3,4,5}, offsets ~ U(+-spline_amp), first waypoint = start
   * position, natural cubic spline sampled at max_episode_steps points over spline_duration s. */
  float spline_center_low[3], spline_center_high[3], spline_amp[3];
  float spline_duration;        /* 30 */
} QuadCfg;

/* Env state in field-major SoA: each array is [fields][N] (qpos [11][N], qvel [10][N], ...).
 * qpos = MuJoCo qpos (x y z qw qx qy qz theta1..4), qvel = MuJoCo qvel (world v, body omega,
 * prop rates); voltage = HoverEnv.voltage; target = target_state.position; rate_int =
 * RateControlWrapper._rate_int_torque; step_count = HoverEnv._step_count; episode = the number of
 * resets drawn so far (the reset RNG counter); prev_action = HoverEnv._prev_action [4][N] (kept for
 * QUAD_WRAP_RELPOS). NULL members are skipped by get/set. */
typedef struct QuadStateSoA {
  float* qpos;
  float* qvel;
  float* voltage;
  float* target;
  float* rate_int;
  int32_t* step_count;
  uint32_t* episode;
  float* prev_action;
} QuadStateSoA;

/* Outputs of quad_step (device pointers). Required: obs, reward, terminated, truncated.
 *  obs            [N,12] normalized observation (after auto-reset for envs that finished);
 *                        brax kinds: [N,21] raw [qpos, qvel]
 *  reward         [N]    exp(-|pos - target|^2)           (hover_env.py:138-141)
 *  terminated     [N]    NaN / state-bounds termination   (hover_env.py:150-157)
 *  truncated      [N]    step_count >= max_episode_steps  (hover_env.py:188)
 * Optional (NULL to skip):
 *  terminal_obs   [N,12|21] obs before auto-reset (SB3 info["terminal_observation"]); only rows of
 *                        envs that finished this step are written
 *  motor_commands [N,4]  info["motor_commands"] (N)
 *  voltage_scale  [N]    info["voltage_scale"]
 *  state12        [N,12] info["state"]: absolute 12-D QuadState before auto-reset
 *  target_info    [N,9]  info["target"], ["target_vel"], ["target_acc"] before auto-reset: the
 *                        TrajectoryFollowEnv spline sample at min(step - 1, L - 1)
 *                        (trajectory_follow_env.py:163-168; regenerated from the episode's reset
 *                        draw, so it follows quad_reset/auto-reset episodes, not injected states);
 *                        the fixed target and zeros for the hover kinds */
typedef struct QuadStepOut {
  float* obs;
  float* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  float* terminal_obs;
  float* motor_commands;
  float* voltage_scale;
  float* state12;
  float* target_info;
} QuadStepOut;

typedef struct QuadHandle QuadHandle;

int quad_abi_version(void);
const char* quad_last_error(void);

/* Fill `cfg` with the reference defaults for (env_kind, wrapper); auto_reset = 1. */
int quad_default_cfg(int32_t env_kind, int32_t wrapper, QuadCfg* cfg);

/* Allocate N envs on `device`. Global env ids are env_id_base .. env_id_base+N-1; the reset RNG
 * is Philox4x32-10 keyed by `seed` with counter (global env id, episode, draw block), so a
 * shard's trajectories do not depend on how many GPUs the envs are spread over.
 * State starts zeroed; call quad_reset before stepping. 1 <= N <= 33,554,431 (the state SoA is
 * addressed as one 4 GiB buffer resource); QUAD_EINVAL otherwise. */
int quad_create(const QuadCfg* cfg, int32_t device, uint64_t seed, uint64_t env_id_base,
                int32_t n_envs, QuadHandle** out);
void quad_destroy(QuadHandle* h);
int32_t quad_num_envs(const QuadHandle* h);
/* Diagnostics: the step-kernel form quad_create chose -- bit 4 set when the handle's constant block
 * is a reference default and the kernels with compiled-in constants run (QUADENV_SPEC=0 turns that
 * off), bit 5 always set for the hover / trajectory kinds (one thread per env with helper waves
 * drawing the resets, k_step_h; bits 0-3 were the lane-group forms removed in round 6), bit 7 set when those helper blocks are 256 envs wide (full-batch steps of 32,769 .. 2,097,151 envs,
 * or QUADENV_HBLOCK=256; 64-env blocks otherwise), bit 8 set when a full-batch step of those blocks
 * moves the env state with the nt cache policy (65,536-env-scale and >= 2M-env batches; QUADENV_NT
 * pins it), bit 9 set when those 64-env nt launches run as k_step_hd, the DRAM form with a
 * 7-waves-per-SIMD register budget (>= 4M-env batches; QUADENV_HD pins it). 64 alone: a RELPOS or brax handle, whose one step kernel (k_step_relpos / k_step_brax) has no forms. */
int32_t quad_kernel_form(const QuadHandle* h);

/* Re-key the reset RNG (HoverEnv.reset(seed=...), hover_env.py:210 -> gymnasium seeding) and
 * zero every env's episode counter (stream-ordered). */
int quad_seed(QuadHandle* h, uint64_t seed, void* stream);

/* HoverEnv.reset for every env (mask == NULL) or for envs with mask[i] != 0 (device [N] u8).
 * Writes the reset observation rows to obs (device [N,12]) when obs != NULL. */
int quad_reset(QuadHandle* h, const uint8_t* mask, float* obs, void* stream);

/* One vectorized env step: actions is device [N,4] float32 in the policy's normalized space
 * (the CTBR wrapper's rate space when wrapper == QUAD_WRAP_CTBR). Not clipped by the env. */
int quad_step(QuadHandle* h, const float* actions, const QuadStepOut* out, void* stream);

/* quad_step restricted to envs [first, first + count): rows of actions/out outside the range are
 * neither read nor written. Sub-ranges on different streams let independent halves of a batch
 * overlap (one half's physics with the other half's memory traffic, or with a policy kernel). */
int quad_step_range(QuadHandle* h, int32_t first, int32_t count, const float* actions,
                    const QuadStepOut* out, void* stream);

/* Measurement only (no reference counterpart; bench.py's live DRAM floor): the HBM traffic of one
 * quad_step with no compute -- the same env tiles, actions and output rows, with quad_step's cache
 * policy for this batch size: every env's 26 state words (qpos 11, qvel 10, voltage, target 3, step
 * counter) read and written back unchanged, its action read, and obs [N,12], reward, terminated and
 * truncated written (obs = the first 12 state words, reward = qpos[0], flags = 0). 278 bytes per env,
 * quad_step's algorithmic bytes. The env state is left as it was; the output rows are overwritten.
 * Hover / trajectory kinds without RELPOS. */
int quad_mem_floor(QuadHandle* h, const float* actions, const QuadStepOut* out, void* stream);

/* HoverEnv._get_obs for the current state (e.g. after quad_set_state). obs: device [N,12];
 * state12 (device [N,12] or NULL): the absolute QuadState vector (HoverEnv._state.vec()). */
int quad_observe(QuadHandle* h, float* obs, float* state12, void* stream);

/* Config 2 of the scope table -- the random-action rollout of debug_training.py:111
 * (env.step(env.action_space.sample()) in a loop) -- as ONE launch: `steps` consecutive quad_step
 * calls with the actions quad_random_actions(step0 + s) gives, the env state kept on chip between
 * steps. Results are identical to quad_random_actions + quad_step, step by step. Every QuadStepOut
 * pointer is time-major: obs [steps][N,12], reward / terminated / truncated [steps][N], terminal_obs
 * [steps][N,12] (optional; rows of envs that finished that step); motor_commands, voltage_scale,
 * state12 and target_info must be NULL. actions_out: [steps][N,4] (16-byte aligned) or NULL.
 * Hover / trajectory kinds, wrapper NONE or CTBR; steps * N * 48 < 2^32. */
int quad_step_random(QuadHandle* h, uint32_t step0, int32_t steps, const QuadStepOut* out, float* actions_out,
                     void* stream);

/* HoverEnv._is_terminated (hover_env.py:150-157; TrajectoryFollowEnv's bounds for that kind) on n
 * caller-given absolute 12-D states (device [n,12], the QuadState vector: pos, roll/pitch/yaw, world
 * velocity, body rates): terminated[i] = any non-finite component or any component outside the
 * handle's inclusive termination bounds -- the predicate quad_step applies after each step.
 * terminated: device [n] u8. Not defined for the brax kinds (QUAD_EINVAL). */
int quad_terminated(QuadHandle* h, const float* state12, int32_t n, uint8_t* terminated, void* stream);

/* action_space.sample() equivalent for synthetic rollouts: U[-1,1)^4 per env from
 * Philox(seed, global env id, step_index). actions: device [N,4]. */
int quad_random_actions(QuadHandle* h, uint32_t step_index, float* actions, void* stream);

/* Copy the env state out of / into the handle. `on_host` != 0: the SoA arrays are host memory
 * (the call synchronizes `stream`); otherwise device memory (async). */
int quad_get_state(QuadHandle* h, const QuadStateSoA* dst, int32_t on_host, void* stream);
int quad_set_state(QuadHandle* h, const QuadStateSoA* src, int32_t on_host, void* stream);

/* ---- Batched waypoint-following evaluation (row f4): evaluate.py:440-612 evaluate_trajectory
 * for N envs at once (hover / trajectory kinds, any wrapper). Waypoint sets are float64 (the
 * generators' numpy arrays) [n_sets][max_points][3]; env i follows set set_of[i] (0 if NULL). */
typedef struct QuadWaypoints {
  const double* points;    /* device [n_sets][max_points][3] */
  const int32_t* counts;   /* device [n_sets], >= 1 */
  const int32_t* set_of;   /* device [N] or NULL */
  int32_t max_points;
  float reach_radius;      /* --reach-radius (0.25) */
} QuadWaypoints;
/* Per-env tracker (device [N] arrays). status: 0 running, 1 lap completed, 2 terminated,
 * 3 truncated (max steps). */
typedef struct QuadWaypointState {
  int32_t* wp_idx;
  int32_t* reached;
  int32_t* laps;
  int32_t* steps;
  int32_t* status;
  double* total_reward;
} QuadWaypointState;
/* Start every env at its first waypoint (evaluate.py:487-505): qpos[0:7] = (wp0, 1, 0, 0, 0),
 * qvel[0:6] = 0 (props keep their reset state), target = wp[1 % n], rate integrator 0, step 0;
 * tracker zeroed with wp_idx = 1 % n; writes the observation (HoverEnv._get_obs, or the
 * RelPosActWrapper observation) to obs. Call after quad_reset. */
int quad_waypoints_begin(QuadHandle* h, const QuadWaypoints* w, const QuadWaypointState* s, float* obs,
                         void* stream);
/* After each quad_step (create the handle with auto_reset = 0): for envs still running, add the
 * reward, count the step, switch to the next waypoint when |pos - wp| < reach_radius (pos =
 * the step's state12[:, 0:3], info["state"]); completing the lap, terminated or truncated end
 * the env's evaluation (evaluate.py:545-595). The next waypoint is written as the env target. */
int quad_waypoints_update(QuadHandle* h, const QuadWaypoints* w, const QuadWaypointState* s,
                          const float* state12, const float* reward, const uint8_t* terminated,
                          const uint8_t* truncated, void* stream);

/* ---- Cascaded PID baseline: the reference's hover controller (pid_controller.py:40-191) and its
 * trajectory-following sibling (pid_controller_world_frame.py:86-283), batched, with one gain set per
 * env. Hover / trajectory kinds, wrapper NONE (the law emits the normalized thrust / torque action). */
enum { QUAD_PID_YAW_FRAME = 0,     /* pid_controller.py: no feed-forward, yaw-only rotation, yaw setpoint 0 */
       QUAD_PID_WORLD_FRAME = 1 }; /* _world_frame.py: velocity-error D term, acceleration feed-forward,
                                      Z-Y-X Euler rotation, yaw toward the target velocity's heading */
/* The 21 numbers CascadedPIDController.__init__ reads from pid_gains.json, in its order, and the one
 * plant constant of the law the handle's QuadCfg does not hold (drone_config.py MASS). The others come
 * from the handle: G = -gravity[2], DT = timestep, MAX_TOTAL_THRUST = 4 max_motor_thrust, MAX_TORQUE =
 * max_torque, ARM_LENGTH = arm_length, IXX / IYY / IZZ = inertia[]. */
typedef struct QuadPidGains {
  double kp_xy, kd_xy, ki_xy;               /* position_xy */
  double kp_z, kd_z, ki_z;                  /* position_z */
  double kp_att, kd_att;                    /* attitude */
  double kp_yaw, kd_yaw;                    /* yaw */
  double ki_rate_torque, rate_int_max;      /* rate: ki_torque, integral_max */
  double axy_max, az_min, az_max, tilt_max; /* limits */
  double z_int_max, xy_int_max;             /* limits: z_integral_max, xy_integral_max */
  double torque_motor_frac, torque_abs_max, yaw_torque_scale; /* limits: torque_motor_fraction, ... */
  double mass;                              /* drone_config.py MASS (0.2227) */
} QuadPidGains;
/* pid_gains.json's committed values and MASS. */
int quad_pid_default_gains(QuadPidGains* g);

/* One CascadedPIDController.compute per row, float64 on the float32 inputs: state12 [n,12] (info["state"]),
 * target9 [n,9] (info["target"], ["target_vel"], ["target_acc"]; the yaw-frame law reads the first three),
 * row i with gain set set_of[i] (0 if set_of is NULL) of the device table gains[n_sets]. integ: device
 * float64 [6][n], field-major (xy integral 2, z integral, rate-torque integral 3), read and updated
 * (zero it where the reference calls controller.reset()). actions: [n,4] float32, clipped to [-1, 1].
 * diag (NULL to skip): float64 [n,6] = des_rate 3, des_att 3. A row whose set_of entry is outside
 * [0, n_sets) reads no gain set: its action is zero and its integrators are left as they were. */
int quad_pid_act(QuadHandle* h, const QuadPidGains* gains, int32_t n_sets, const int32_t* set_of, int32_t mode,
                 const float* state12, const float* target9, int32_t n, double* integ, float* actions,
                 double* diag, void* stream);

/* info["target"], ["target_vel"], ["target_acc"] as the env's reset / last step reported them, for the
 * current step count (target_info [N,9]; hover / trajectory kinds): what a host loop hands the law
 * before its first quad_step, next to quad_observe's state12. */
int quad_target_info(QuadHandle* h, float* target_info, void* stream);

/* Per-env episode metrics (device [N] arrays, all required), accumulated as auto_tune_pid.py:66-124
 * reads them from info["state"] after each step. status: 0 still running after max_steps iterations,
 * 1 terminated, 2 truncated, 3 invalid (set_of out of range: no step taken). */
enum { QUAD_PID_RUNNING = 0, QUAD_PID_TERMINATED = 1, QUAD_PID_TRUNCATED = 2, QUAD_PID_INVALID = 3 };
typedef struct QuadPidMetrics {
  int32_t* steps;
  int32_t* status;
  double* total_reward;
  double* pos_err_sum;      /* sum of |pos after the step - target read before it| (float32 difference) */
  double* pos_err_sq;       /* sum of its squares */
  double* pos_err_max;
  double* yaw_rate_abs_sum; /* yaw rate = state[11] */
  double* yaw_rate_sum;
  double* yaw_rate_sq;
  double* yaw_rate_abs_max;
  int32_t* yaw_rate_sign_changes; /* steps whose np.sign(yaw rate) differs from the step before (zeros count) */
  double* yaw_rate_delta_sum;     /* sum of |yaw rate - yaw rate of the step before| */
} QuadPidMetrics;

/* The fused closed loop, ONE launch: every env runs (law -> HoverEnv.step) until its first terminated or
 * truncated step or for max_steps iterations, its state in registers throughout; it is then frozen (no
 * reset) and its state after its last step is stored. The law's inputs are what quad_observe /
 * quad_target_info report before the first step and the step's own state12 / target_info afterwards --
 * the loop of pid_controller.py:434-439. Bit-identical to quad_pid_act + quad_step per step on a handle
 * with auto_reset = 0. integ (NULL: start from zero, not stored): float64 [6][N] in / out.
 * Traces (NULL to skip) are time-major for the first trace_envs envs: trace_actions
 * [max_steps][trace_envs,4], trace_state12 [max_steps][trace_envs,12]; rows past an env's last step are
 * not written; max_steps * trace_envs * 48 < 2^32. */
typedef struct QuadPidRun {
  const QuadPidGains* gains; /* device [n_sets] */
  const int32_t* set_of;     /* device [N] or NULL (set 0) */
  int32_t n_sets;            /* >= 1 */
  int32_t mode;              /* QUAD_PID_YAW_FRAME | QUAD_PID_WORLD_FRAME */
  int32_t max_steps;         /* >= 1 */
  int32_t trace_envs;        /* 0 .. N */
  double* integ;
  float* trace_actions;
  float* trace_state12;
  QuadPidMetrics metrics;
} QuadPidRun;
int quad_pid_episode(QuadHandle* h, const QuadPidRun* r, void* stream);

/* ---- The controller family: the reference's other three classical controllers beside the PID, as
 * fused batched laws of the same shape. Each law is one compute() call of its reference class, quirks
 * included. The two PID ids run quad_pid_act's law, so this family is a superset. */
enum { QUAD_CTRL_PID_YAW = 0,   /* = QUAD_PID_YAW_FRAME */
       QUAD_CTRL_PID_WORLD = 1, /* = QUAD_PID_WORLD_FRAME */
       QUAD_CTRL_SE3 = 2,       /* se3_geometric_controller.py:247-426 */
       QUAD_CTRL_SMC = 3,       /* smc_controller_world_frame.py:146-322 */
       QUAD_CTRL_LQR = 4 };     /* lqr_controller_world_frame.py:139-289 */
#define QUAD_CTRL_NSTATE 8 /* rows of the controller-state block */
#define QUAD_CTRL_NDIAG 7  /* diag columns */
/* 33 doubles: the shared gain set, then what only one law reads. */
typedef struct QuadCtrlParams {
  QuadPidGains base;
  double lqr_k[3];                   /* LQR: K[0,0], K[0,1], K[0,2]; default [1 + sqrt 2, 1 + sqrt 2, 1] */
  double yaw_stw_k1, yaw_stw_k2;     /* SMC super-twisting yaw loop: 1.2, 2.0 */
  double yaw_stw_boundary;           /* 0.05 */
  double yaw_deadband;               /* deg2rad(1) */
  double yaw_v_int_max;              /* 2.0 */
  double yaw_rate_max;               /* 3.0 */
  double yaw_rate_lpf_alpha;         /* 0.2 */
  double se3_reorthonormalize;       /* SE(3): non-zero (default 1) passes R_desired through np.linalg.qr's
                                        Householder Q as the reference does; 0 uses [x_d y_d z_d] as built */
} QuadCtrlParams;
int quad_ctrl_default_params(QuadCtrlParams* p);

/* quad_pid_act for any law. state: device float64 [8][n], field-major: the six integrators in
 * quad_pid_act's order, then v_yaw and des_wz_prev (SMC; the other laws leave rows 6-7 untouched).
 * diag (NULL to skip): float64 [n,7] = des_rate 3, des_att 3, |e_R| (SE(3); 0 otherwise). A row whose
 * set_of entry is outside [0, n_sets) reads no parameter set: zero action, state left as it was. */
int quad_ctrl_act(QuadHandle* h, const QuadCtrlParams* params, int32_t n_sets, const int32_t* set_of, int32_t law,
                  const float* state12, const float* target9, int32_t n, double* state, float* actions,
                  double* diag, void* stream);

/* quad_pid_episode for any law: QuadPidRun's fields and rules, with the law, the parameter table and the
 * [8][N] state block (NULL: start from zero, not stored). Bit-identical to quad_ctrl_act + quad_step per
 * step on a handle with auto_reset = 0, and, with a PID law, to quad_pid_episode. */
typedef struct QuadCtrlRun {
  const QuadCtrlParams* params; /* device [n_sets] */
  const int32_t* set_of;        /* device [N] or NULL (set 0) */
  int32_t n_sets;               /* >= 1 */
  int32_t law;                  /* QUAD_CTRL_* */
  int32_t max_steps;            /* >= 1 */
  int32_t trace_envs;           /* 0 .. N */
  double* state;
  float* trace_actions;
  float* trace_state12;
  QuadPidMetrics metrics;
} QuadCtrlRun;
int quad_ctrl_episode(QuadHandle* h, const QuadCtrlRun* r, void* stream);

/* ---- The deployed observation path and the policy's fused episode. The reference deploys the
 * policy through ros2_ws policy_node.py, which does not feed it the env's observation: the linear velocity
 * is state_estimator.VelocityEstimator's -- a first-order low-pass (velocity_alpha, default 0.8) on finite
 * differences of the mocap position -- and observation_builder.build_observation clips the normalised
 * vector to [-1, 1]. QuadVelEst is one estimator per env. */
enum { QUAD_OBS_ENV = 0, QUAD_OBS_DEPLOYED = 1 };
#define QUAD_EST_NSTATE 8 /* rows of the estimator block: prev_pos 3, prev_time, velocity 3, has_prev (0 / 1) */
typedef struct QuadVelEst {
  const double* alpha;  /* device [N] or NULL (alpha_all for every env) */
  double alpha_all;     /* policy_node.py default 0.8 */
  double max_dt;        /* 0.1 */
  double* state;        /* device float64 [8][N] field-major in/out; NULL: start empty, not stored */
} QuadVelEst;

/* One VelocityEstimator.update(position, timestamp) and one build_observation per row: state12 [n,12]
 * (position, attitude, velocity, body rates; the velocity columns are NOT read), target3 [n,3]; writes
 * obs [n,12] and, unless NULL, vel_est [n,3] (the estimate rounded to float32, as obs holds it before
 * normalisation). The observation bounds are the handle's. est->state is required (zero it to start). */
int quad_deploy_obs(QuadHandle* h, const QuadVelEst* est, const float* state12, const float* target3,
                    double timestamp, int32_t n, float* obs, float* vel_est, void* stream);

/* quad_deploy_obs with one timestamp per row (device float64 [n]) and a code per row (device uint8 [n], or NULL:
 * every row is 1), for a batch whose envs sit at different step counts and reset at different times:
 *   0  the row is skipped: its estimator state, its obs row and its vel_est row stay untouched
 *   1  the row is updated, as quad_deploy_obs updates it
 *   2  the row's eight estimator words are set to zero first (a new VelocityEstimator), then it is updated
 * Any other code is undefined (not checked on the device). The same two functions as quad_deploy_obs: with equal
 * timestamps and rows == NULL it is bit-identical to it. The same argument checks, and timestamps is required. */
int quad_deploy_obs_rows(QuadHandle* h, const QuadVelEst* est, const float* state12, const float* target3,
                         const double* timestamps, const uint8_t* rows, int32_t n, float* obs, float* vel_est,
                         void* stream);

/* The deterministic policy's whole episodes in ONE launch from the envs' current state: per step the actor
 * (MFMA), clip(mean, -1, 1), the env step, QuadPidRun's metrics, the estimator update and its error. Every
 * env runs until its first terminated / truncated step or max_steps and is then frozen, never reset (the
 * handle's auto_reset setting is not consulted). The estimator sees the position in hand before the first
 * action at timestamp step_count * est_dt, then each step's position at the new step count.
 * vel_err_sq[i] = sum over env i's steps of |v_est - state12[6:9]|^2 after the step (float64).
 * Traces, time-major [max_steps, trace_envs, .] of the first trace_envs envs, rows past an env's last step
 * untouched: actions (the clipped action, 16-byte aligned), obs (the observation that action was taken
 * from), state12 and vel_est (after the step). Requires env_kind HOVER or TRAJ, wrapper NONE or CTBR.
 * Contract: bit-identical, for every env up to its last step, to this loop on a second handle:
 * quad_observe, then quad_deploy_obs at the reset step count, once; per step quad_policy_act with
 * deterministic = 1, quad_step, and quad_deploy_obs on the step's state12 (target3 = the env's target)
 * at the new step count -- the act reading quad_observe's / quad_step's obs in QUAD_OBS_ENV and
 * quad_deploy_obs's in QUAD_OBS_DEPLOYED. */
typedef struct QuadPolicyRun {
  int32_t obs_mode;     /* QUAD_OBS_ENV: the policy sees the env's observation, the estimator runs beside it;
                           QUAD_OBS_DEPLOYED: the policy sees deploy_obs */
  int32_t max_steps, trace_envs;
  QuadVelEst est; double est_dt;            /* timestamp of step count k = k * est_dt */
  float *trace_actions, *trace_state12, *trace_obs, *trace_vel_est;  /* time-major, first trace_envs envs, NULL to skip */
  QuadPidMetrics metrics;                   /* all required, QuadPidRun's rules and status codes */
  double* vel_err_sq;                       /* [N] or NULL */
} QuadPolicyRun;
int quad_policy_episode(QuadHandle* h, const float* packed, const QuadPolicyRun* r, void* stream);

/* ---- Waypoint laps in ONE launch: evaluate.py:440-612 evaluate_trajectory for the policy and
 * for every law of the controller family. Call after quad_waypoints_begin (or an earlier run: s is in / out).
 * Every env whose tracker status is 0 runs (law or actor -> env step -> tracker) until its tracker status
 * leaves 0 or for max_steps iterations and is then frozen, as in quad_ctrl_episode; an env that enters with
 * another status takes no step. A switch overwrites the env's target register, so the handle must be of the
 * HOVER kind (the reference builds a HoverEnv); wrapper NONE for the laws, NONE or CTBR for the policy.
 * reach_radius >= 0 (0: no waypoint is ever reached, the distance test is strict).
 * The metrics' status is QUAD_PID_LAP where the tracker's is 1, TERMINATED / TRUNCATED where it is 2 / 3,
 * RUNNING where it is still 0, and QUAD_PID_INVALID for an env whose QuadCtrlRun set_of entry is out of
 * range: that env takes no step and its tracker row is left as it was. The metrics restart from zero in
 * every call; the tracker's steps and total_reward carry on. The position error uses the target read before
 * the step. Controller and estimator state carry across switches: nothing resets them.
 * Traces: the run's own (QuadCtrlRun / QuadPolicyRun) plus trace_reward [max_steps][trace_envs] and
 * trace_wp_idx [max_steps][trace_envs], the index of the waypoint the step flew toward; the run's
 * max_steps * trace_envs bound applies.
 * Contract: bit-identical, for every env up to its last step, to this loop on a second handle with
 * auto_reset = 0: quad_observe and quad_target_info once; per step quad_ctrl_act (or quad_policy_act with
 * deterministic = 1), quad_step, quad_waypoints_update, quad_target_info. In QUAD_OBS_ENV the policy acts on
 * quad_step's observation, which is built with the target the step was flown with -- one step stale after a
 * switch, as evaluate.py:537-555 has it. In QUAD_OBS_DEPLOYED it acts on quad_deploy_obs called after the
 * tracker update with the env's new target: the node always reads the current setpoint. */
#define QUAD_PID_LAP 4 /* joins QUAD_PID_RUNNING .. QUAD_PID_INVALID */
typedef struct QuadWaypointRun {
  QuadWaypoints w;
  QuadWaypointState s;    /* in/out: as quad_waypoints_begin (or an earlier run) left it */
  float*   trace_reward;  /* [max_steps][trace_envs] or NULL */
  int32_t* trace_wp_idx;  /* the waypoint index the step flew toward, or NULL */
} QuadWaypointRun;
int quad_ctrl_waypoints(QuadHandle* h, const QuadCtrlRun* r, const QuadWaypointRun* wr, void* stream);
int quad_policy_waypoints(QuadHandle* h, const float* packed, const QuadPolicyRun* r, const QuadWaypointRun* wr,
                          void* stream);

/* PPO rollout support (row P of the scope table): generalized advantage estimation over a
 * time-major rollout, SB3 RolloutBuffer.compute_returns_and_advantage semantics.
 *  rewards, values, episode_starts: device [T,N] float32 (episode_starts 1.0 where the step
 *  began a new episode); last_values [N]; dones [N] (1.0 if the env finished at the last step).
 *  Writes advantages and returns (= advantages + values), device [T,N]. */
int quad_gae(const float* rewards, const float* values, const float* episode_starts,
             const float* last_values, const float* dones, int32_t T, int32_t N, float gamma,
             float gae_lambda, float* advantages, float* returns, void* stream);

/* ---- Rollout policy on MFMA (row P): the SB3 ActorCritic that train.py:50-68 configures
 * (MlpPolicy, net_arch pi=[128,128] vf=[128,128], ReLU, state-independent log_std), fp32.
 * Parameter pointers are device fp32 in torch's nn.Linear layout ([out, in] row-major). */
typedef struct QuadPolicyParams {
  const float *pi_w0, *pi_b0, *pi_w1, *pi_b1;  /* mlp_extractor.policy_net.{0,2} [128,12] [128,128] */
  const float *act_w, *act_b;                  /* action_net [4,128] [4] */
  const float *vf_w0, *vf_b0, *vf_w1, *vf_b1;  /* mlp_extractor.value_net.{0,2} */
  const float *val_w, *val_b;                  /* value_net [1,128] [1] */
  const float* log_std;                        /* [4] */
} QuadPolicyParams;

/* Size (floats) of the packed policy image quad_policy_pack writes. */
int32_t quad_policy_packed_floats(void);

/* Repack the parameters into the MFMA fragment order the policy kernels read (call after every
 * optimizer update that precedes a rollout; stream-ordered). `packed`: device, 16-byte aligned. */
int quad_policy_pack(const QuadPolicyParams* p, float* packed, void* stream);

/* Rollout epilogue of one step (after quad_step), SB3 collect_rollouts semantics:
 * buf_rew[row] = reward + gamma * V(terminal_obs) where truncated && !terminated (TimeLimit
 * bootstrap; the critic runs only on 32-env tiles that hold such an env), else reward;
 * last_start = terminated | truncated; Monitor statistics: ep_ret/ep_len accumulate and reset on
 * done, stats[slot] += (finished return, length, 1) -- sum the QUAD_POLICY_STAT_SLOTS slots. */
enum { QUAD_POLICY_STAT_SLOTS = 1024 };
typedef struct QuadRolloutPost {
  const float* reward;          /* [N] */
  const uint8_t* terminated;    /* [N] */
  const uint8_t* truncated;     /* [N] */
  const float* terminal_obs;    /* [N,12] */
  float* buf_rew;               /* [rows,N] */
  float* last_start;            /* [N] */
  float* ep_ret;                /* [N] running episode return */
  float* ep_len;                /* [N] running episode length */
  double* stats;                /* [QUAD_POLICY_STAT_SLOTS][3], zeroed by the caller */
  int32_t rows;
  float gamma;
} QuadRolloutPost;

/* One rollout-step policy evaluation (SB3 OnPolicyAlgorithm.collect_rollouts body):
 * a = mean(obs) + exp(log_std) * z, z ~ N(0,1) from Philox(seed; env id, t, 0x200) + Box-Muller;
 * actions_env = clip(a, -1, 1). `cursor` (device uint32[4] = {t, pending, 0, 0}, zero it to start)
 * holds the running step counter t (never reset, so successive rollouts draw fresh noise); row
 * outputs go to row t % rows of time-major [rows,N,...] buffers; every row pointer may be NULL.
 * With `epilogue` != NULL the launch first finishes step t-1 if it is pending (QuadRolloutPost
 * above, row (t-1) % rows, before episode_starts[t] is taken from last_start), then advances the
 * cursor to t+1 and marks step t pending: one launch per step besides quad_step. */
typedef struct QuadPolicyAct {
  const float* obs;         /* [N,12] */
  float* actions_env;       /* [N,4] clipped action for quad_step (16-byte aligned) */
  float* actions;           /* [rows,N,4] unclipped sample (rollout buffer) or NULL */
  float* log_prob;          /* [rows,N] or NULL */
  float* value;             /* [rows,N] critic V(obs) or NULL */
  float* obs_copy;          /* [rows,N,12] or NULL */
  const float* last_start;  /* [N] episode_starts of this step or NULL */
  float* episode_starts;    /* [rows,N] or NULL */
  uint32_t* cursor;         /* device uint32[4] or NULL (t = 0, read-only without epilogue) */
  int32_t rows;             /* >= 1 */
  int32_t deterministic;    /* 1: a = mean (policy.predict(deterministic=True)) */
  uint64_t seed;
  uint64_t env_id_base;     /* global id of env 0 (keys the noise per env, shard-independent) */
  const QuadRolloutPost* epilogue;  /* fused epilogue of step t-1, or NULL */
} QuadPolicyAct;
int quad_policy_act(const float* packed, const QuadPolicyAct* a, int32_t n, void* stream);

/* ---- A deterministic actor of any supported architecture on MFMA: mean = W3 act(W2 act(W1 x +
 * b1) + b2) + b3 with 12-D observations and 4 outputs, h1 a multiple of 32 in [32, 512], h2 in {64, 128, 256},
 * act ReLU or tanh -- the reference's optimize.py family and SB3's MlpPolicy default. Forward path only (no
 * critic, no sampling, no log-probs): evaluation episodes, waypoint laps, the deployed observation path.
 * The arithmetic is quad_policy_act's (three-piece bf16 splits, six piece products, f32 accumulation).
 * Parameter pointers are device fp32 in torch's nn.Linear layout ([out, in] row-major): w0 [h1,12] b0 [h1]
 * w1 [h2,h1] b1 [h2] w2 [4,h2] b2 [4]. An arch outside the family is QUAD_EINVAL (quad_actor_packed_floats: < 0).
 * The added entry points did not change the ABI version. */
enum { QUAD_ACTFN_RELU = 0, QUAD_ACTFN_TANH = 1 };
typedef struct QuadActorArch { int32_t h1, h2, activation; } QuadActorArch;
typedef struct QuadActorParams { const float *w0, *b0, *w1, *b1, *w2, *b2; } QuadActorParams;
/* Size (floats) of the packed image quad_actor_pack writes for this arch. */
int64_t quad_actor_packed_floats(const QuadActorArch* arch);
/* Repack the parameters into the fragment order the actor kernels read (stream-ordered). `packed`: device,
 * 16-byte aligned, quad_actor_packed_floats(arch) floats. */
int quad_actor_pack(const QuadActorArch* arch, const QuadActorParams* p, float* packed, void* stream);
/* mean [n,4] (or NULL) and actions_env [n,4] = clip(mean, -1, 1) (16-byte aligned; a NaN mean gives -1) of
 * obs [n,12]. A row's result does not depend on n or on the other rows. */
int quad_actor_act(const QuadActorArch* arch, const float* packed, const float* obs, float* mean,
                   float* actions_env, int32_t n, void* stream);
/* quad_policy_episode / quad_policy_waypoints with this actor: the same semantics, argument checks, status
 * codes and trace rules, and the same contract -- bit-identical, for every env up to its last step, to their
 * loops on a second handle with quad_actor_act in quad_policy_act's place. `packed`: quad_actor_pack's image. */
int quad_actor_episode(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadPolicyRun* r,
                       void* stream);
int quad_actor_waypoints(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadPolicyRun* r,
                         const QuadWaypointRun* wr, void* stream);

/* ---- The Brax-profile policy on MFMA: ppo/brax_ppo.py BraxActorCritic.policy with two hidden layers on
 * the 21-D observation of the brax env kinds, logits[8] = W3 act(W2 act(W1 xh + b1) + b2) + b3 with
 * xh = (obs - mean) / std in f32 (RunningStats.normalize), h1 a multiple of 32 in [32, 512], h2 in {64, 128, 256},
 * act ReLU, tanh or SiLU; loc = logits[0:4], scale = softplus(logits[4:8]) + min_std (NormalTanhDistribution).
 * quad_actor_act's arithmetic. Forward path only (evaluation); no log-probs, no critic. Kernels are device fp32 in
 * flax's [in, out] layout (BraxMLP.kernels): w0 [21,h1] b0 [h1] w1 [h1,h2] b1 [h2] w2 [h2,8] b2 [8]; mean, std [21].
 * An arch outside the family is QUAD_EINVAL (quad_brax_actor_packed_floats: < 0). Added within ABI v8. */
enum { QUAD_ACTFN_SILU = 2 };
typedef struct QuadBraxActorArch { int32_t h1, h2, activation; } QuadBraxActorArch;
typedef struct QuadBraxActorParams {
  const float *w0, *b0, *w1, *b1, *w2, *b2, *mean, *std;
  float min_std;
} QuadBraxActorParams;
int64_t quad_brax_actor_packed_floats(const QuadBraxActorArch* arch);
/* `packed`: device, 16-byte aligned, quad_brax_actor_packed_floats(arch) floats (stream-ordered). */
int quad_brax_actor_pack(const QuadBraxActorArch* arch, const QuadBraxActorParams* p, float* packed, void* stream);
/* logits [n,8] (or NULL) and actions_env [n,4] (16-byte aligned) of obs [n,21]: deterministic != 0: tanh(loc);
 * otherwise tanh(loc + scale z), z the four Box-Muller normals of Philox(seed; env_id_base + row, noise_step, 0x400).
 * A row's result depends on neither n nor the other rows; a non-finite row stays in its row. */
int quad_brax_actor_act(const QuadBraxActorArch* arch, const float* packed, const float* obs, float* logits,
                        float* actions_env, int32_t n, int32_t deterministic, uint64_t seed, uint64_t env_id_base,
                        uint32_t noise_step, void* stream);
/* Per-env episode metrics of quad_brax_episode (device [N] arrays, all required), as evaluate_brax_ppo.py:315-362
 * accumulates them. status: QUAD_PID_RUNNING / TERMINATED / TRUNCATED. */
typedef struct QuadBraxMetrics {
  double* ret;          /* sum of the rewards in step order */
  int32_t* steps;
  double* err_sum;      /* sum of |pos - target| (float32 norm) after the step, with the step's target, where finite */
  double* err_sq_sum;   /* sum of its squares */
  int32_t* err_count;   /* steps whose error was finite */
  int32_t* status;
} QuadBraxMetrics;
/* Whole episodes in ONE launch from the envs' current state, on a handle of kind QUAD_ENV_BRAX_HOVER or _BRAX_TRAJ:
 * per step the observation (what quad_observe / quad_step report), the actor, the env step, the metrics. Every env
 * runs until its first terminated or truncated step or for max_steps iterations; it is then frozen and never reset
 * (auto_reset is not consulted). Step t draws its noise with noise_step0 + t and env id = the handle's env_id_base +
 * env. Traces (NULL to skip), time-major [max_steps, trace_envs, .] of the first trace_envs envs, rows past an env's
 * last step untouched: actions (4, 16-byte aligned), obs (21, the row the action was taken from), pos and target (3
 * each, after the step); max_steps * trace_envs * 84 < 2^32.
 * Contract: bit-identical, for every env up to its last step, to this loop on a second handle with auto_reset = 0:
 * quad_observe once; per step quad_brax_actor_act (same deterministic, seed, env_id_base, noise_step0 + t), then
 * quad_step. */
typedef struct QuadBraxRun {
  int32_t max_steps, trace_envs, deterministic;
  uint32_t noise_step0;
  uint64_t seed;
  QuadBraxMetrics metrics;
  float *trace_actions, *trace_obs, *trace_pos, *trace_target;
} QuadBraxRun;
int quad_brax_episode(QuadHandle* h, const QuadBraxActorArch* arch, const float* packed, const QuadBraxRun* r,
                      void* stream);

/* ---- The Brax learner's unrolls: sampled actions with their behaviour log-probs, per step in two
 * launches or `steps` whole steps of ppo/brax_ppo.py BraxPPO._unrolls in one. Added within ABI v8.
 *
 * quad_brax_actor_sample: quad_brax_actor_act for sampled actions, with two more outputs per row.
 * raw [n,4] = loc + scale z, the value the env action's tanh is taken of; log_prob [n] =
 * NormalTanh.log_prob(logits, raw), computed from raw (not from z) with the expression the loss evaluates later:
 * sum over the four components of -1/2 ((raw - loc) / scale)^2 - 1/2 log 2 pi - log scale
 * - 2 (log 2 - raw - softplus(-2 raw)), in f32, every operation rounded on its own. Noise: quad_brax_actor_act's
 * stream and key, so for equal arguments logits and actions_env (= tanh(raw), quad_brax_actor_act's tanh: within
 * 2 ulp of the exact tanh of the stored raw) have quad_brax_actor_act's bits for deterministic = 0. logits (or NULL), raw and
 * actions_env are 16-byte aligned. A row's result depends on neither n nor the other rows. */
int quad_brax_actor_sample(const QuadBraxActorArch* arch, const float* packed, const float* obs, float* logits,
                           float* raw, float* log_prob, float* actions_env, int32_t n, uint64_t seed,
                           uint64_t env_id_base, uint32_t noise_step, void* stream);
/* `steps` whole steps of the learner's unroll loop in ONE launch, on a handle of kind QUAD_ENV_BRAX_HOVER or
 * _BRAX_TRAJ with auto_reset = 1. Step t (0 <= t < steps) of env i writes row t * N + i of the time-major buffers
 * (all required, device): obs [steps,N,21] the observation the action is taken from; raw [steps,N,4] (16-byte
 * aligned) and log_prob [steps,N] as quad_brax_actor_sample gives them with noise step noise_step0 + t and env id =
 * the handle's env_id_base + i; reward; discount = 1 - (terminated | truncated); truncation = truncated &
 * ~terminated (EpisodeWrapper's), as floats. A finished env is reset as quad_step resets it (the first state of its
 * episode) and the next row starts there. After each group of unroll_length steps the current (post-reset)
 * observation goes to next_obs [steps / unroll_length, N, 21].
 * Monitor-style accounting: ep_ret [N] f32, read at entry and written at exit, accumulates an env's rewards; when
 * the env finishes, ep_ret and a count of one are added to stats [QUAD_POLICY_STAT_SLOTS][2] (double: return sum,
 * episodes; the caller zeroes it and sums over the slots) and ep_ret is cleared.
 * Contract: every output, the handle's final state and ep_ret are bit-identical to this loop on a second handle
 * with auto_reset = 1: quad_observe once; per step quad_brax_actor_sample (same seed and env_id_base,
 * noise_step0 + t), then quad_step. The episode count equals the loop's; the return sum may differ by the order of
 * the double additions. QUAD_EINVAL, with nothing launched: another env kind, auto_reset = 0, an arch outside the
 * family, a NULL or misaligned buffer, steps < 1, unroll_length < 1, steps not a multiple of unroll_length,
 * steps * N * 84 >= 2^32 (rows use 32-bit byte offsets). */
typedef struct QuadBraxUnroll {
  float *obs, *raw, *log_prob, *reward, *discount, *truncation;
  float* next_obs;
  float* ep_ret;
  double* stats;
  int32_t steps, unroll_length;
  uint32_t noise_step0;
  uint64_t seed;
} QuadBraxUnroll;
int quad_brax_unroll(QuadHandle* h, const QuadBraxActorArch* arch, const float* packed, const QuadBraxUnroll* u,
                     void* stream);

/* ---- The Brax learner's minibatch gradient: the gradient of ppo/brax_ppo.py brax_ppo_loss (brax's
 * compute_ppo_loss) with respect to the twelve tensors of the policy net 21 -> h1 -> h2 -> 8 and the value net
 * 21 -> h1 -> h2 -> 1, in four launches on `stream` with no host synchronisation. Added within ABI v8.
 *   total = -mean(min(rho A, clip(rho, 1 - eps, 1 + eps) A)) + 0.25 mean((vs - V)^2) - entropy_cost mean(entropy),
 *   rho = exp(NormalTanh.log_prob(logits, raw) - log_prob); (vs, A) = brax's compute_gae of the minibatch's
 *   trajectories on the value net's own baseline and bootstrap V(next_obs), with reward_scaling, discounting,
 *   gae_lambda and the truncation / termination masks (termination = (1 - discount)(1 - truncation)), outside the
 *   gradient; A = (A - mean) / (std(unbiased = False) + 1e-8) over the L mb rows unless normalize_advantage == 0;
 *   entropy = sum of 1/2 + 1/2 log 2 pi + log scale + 2 (log 2 - x - softplus(-2 x)) at ONE sample
 *   x = loc + scale z per row, differentiated through loc and scale.
 * Ties of the min and the clip bounds follow torch's autograd (a tie's gradient is split in half; clamp passes it
 * on the closed interval). Family: policy_h1 = policy_h2 = value_h1 = value_h2 = 128 and QUAD_ACTFN_RELU.
 * Parameters and gradients are device f32 in flax's [in, out] layout (BraxMLP.kernels / biases); the gradients are
 * OVERWRITTEN, not accumulated. mean / std [21]: observations are normalised (obs - mean) / std in f32 with the
 * correctly rounded division (RunningStats.normalize).
 * Batch: the time-major buffers quad_brax_unroll writes -- obs [U,L,N,21], next_obs [U,N,21], raw [U,L,N,4]
 * (16-byte aligned), log_prob / reward / discount / truncation [U,L,N]. Trajectory m = u N + n; its step t is row
 * (u L + t) N + n. index [mb] (int64) names the minibatch's trajectories: each entry must lie in [0, U N) -- this is
 * the CALLER's responsibility, the launches do not check it. Rows are gathered through index; no minibatch copy is
 * made. Row q = t mb + j of the minibatch-ordered arrays below is step t of trajectory index[j].
 * entropy_noise [L,mb,4] (16-byte aligned) is z when given; when NULL z is the four Box-Muller normals of
 * Philox(seed; index[j], noise_step * L + t, 0x500). noise_out [L,mb,4] (or NULL) receives the z used.
 * Diagnostic outputs (NULL to skip): values [L+1,mb] (baseline rows, then the bootstrap row), vs [L,mb],
 * advantages [L,mb] as they enter the surrogate; stats [3] = policy_loss, v_loss, entropy_loss.
 * For equal arguments the results are bit-identical from call to call, and do not depend on where a trajectory's
 * rows lie in the buffers.
 * QUAD_EINVAL, with nothing launched: an arch outside the family; a NULL or misaligned parameter, gradient, unroll
 * buffer or index; a misaligned optional buffer or workspace (16 bytes); mb < 1; L outside [1, 64]; U or N < 1;
 * (L + 1) mb > 2^28; clipping_epsilon <= 0; workspace_bytes < quad_brax_ppo_workspace_bytes(mb, L). */
typedef struct QuadBraxPPOParams {
  const float *pi_w0, *pi_b0, *pi_w1, *pi_b1, *pi_w2, *pi_b2;  /* [21,h1] [h1] [h1,h2] [h2] [h2,8] [8] */
  const float *vf_w0, *vf_b0, *vf_w1, *vf_b1, *vf_w2, *vf_b2;  /* [21,h1] [h1] [h1,h2] [h2] [h2,1] [1] */
  const float *mean, *std;                                     /* [21] */
  float min_std;
  int32_t policy_h1, policy_h2, value_h1, value_h2, activation;
} QuadBraxPPOParams;

typedef struct QuadBraxPPOGrads {
  float *pi_w0, *pi_b0, *pi_w1, *pi_b1, *pi_w2, *pi_b2;
  float *vf_w0, *vf_b0, *vf_w1, *vf_b1, *vf_w2, *vf_b2;
} QuadBraxPPOGrads;

typedef struct QuadBraxPPOBatch {
  const float *obs, *next_obs, *raw, *log_prob, *reward, *discount, *truncation;
  const int64_t* index;        /* [mb] */
  const float* entropy_noise;  /* [L,mb,4] or NULL */
  float* noise_out;            /* [L,mb,4] or NULL */
  float *values, *vs, *advantages;  /* diagnostics, or NULL */
  float* stats;                /* [3] or NULL */
  int32_t U, L, N, mb;
  float clipping_epsilon, entropy_cost, discounting, gae_lambda, reward_scaling;
  int32_t normalize_advantage;
  uint32_t noise_step;
  uint64_t seed;
} QuadBraxPPOBatch;

/* Device workspace (bytes, 16-byte aligned) quad_brax_ppo_grad needs; 0 for mb < 1, L outside [1, 64] or
 * (L + 1) mb > 2^28. */
int64_t quad_brax_ppo_workspace_bytes(int32_t mb, int32_t L);
int quad_brax_ppo_grad(const QuadBraxPPOParams* p, const QuadBraxPPOBatch* b, const QuadBraxPPOGrads* gr,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The same gradient for the Brax actor's whole family. Added within ABI v8. Family: the policy net
 * 21 -> policy_h1 -> policy_h2 -> 8 and the value net 21 -> value_h1 -> value_h2 -> 1, each h1 a multiple of 32 in
 * [32, 512], each h2 in {64, 128, 256} (quad_brax_actor_*'s family), the two nets' sizes independent of each other;
 * one activation for both: QUAD_ACTFN_RELU, QUAD_ACTFN_TANH or QUAD_ACTFN_SILU. The structs, the loss, the layouts,
 * the gather through index, entropy_noise / noise_out (the same Philox draw: for equal arguments noise_out has
 * quad_brax_ppo_grad's bits), the diagnostics and the guarantees are quad_brax_ppo_grad's, in five launches: the
 * gradients are OVERWRITTEN, the results are bit-identical from call to call and do not depend on where a
 * trajectory's rows lie in the buffers, and nothing synchronises with the host. The value loss reads each row's V
 * from the values array the first launch wrote.
 * QUAD_EINVAL, with nothing launched and nothing written: an arch outside the family; a NULL or misaligned
 * parameter, gradient, unroll buffer or index; a misaligned optional buffer or workspace (16 bytes); mb < 1; L
 * outside [1, 64]; U or N < 1; L mb > 2^22 loss rows; clipping_epsilon <= 0; workspace_bytes <
 * quad_brax_ppo_arch_workspace_bytes(p, mb, L). */
/* Device workspace (bytes, 16-byte aligned) quad_brax_ppo_arch_grad needs for p's four sizes and activation (its
 * pointers are not read); 0 for p NULL or outside the family, mb < 1, L outside [1, 64] or L mb > 2^22. It holds the
 * x | 1, h1, dh2 and dh1 images of every loss row: about 4 (32 + 2 h1 + h2) bytes per row and net. */
int64_t quad_brax_ppo_arch_workspace_bytes(const QuadBraxPPOParams* p, int32_t mb, int32_t L);
int quad_brax_ppo_arch_grad(const QuadBraxPPOParams* p, const QuadBraxPPOBatch* b, const QuadBraxPPOGrads* gr,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* Finish the pending step (end of a rollout): the epilogue for row (t-1) % rows if the cursor
 * marks one pending, then clears the mark. A no-op otherwise. */
int quad_rollout_post(const float* packed, const QuadRolloutPost* p, uint32_t* cursor, int32_t n,
                      void* stream);

/* ---- Fused rollout: `steps` whole steps of SB3 OnPolicyAlgorithm.collect_rollouts (train.py:50-68
 * drives it through SB3's PPO.learn) in ONE launch -- per step: policy (both MLPs on MFMA,
 * Gaussian sample, log-prob, clip), the env step of the handle (HoverEnv / TrajectoryFollowEnv,
 * optional RateControlWrapper, SB3 auto-reset), TimeLimit bootstrap, Monitor statistics, buffer
 * rows. Each 256-env block keeps its envs' state in registers and the packed weights in LDS for
 * all `steps`, so per step nothing is read from HBM. Results are bit-identical to the two-launch
 * form (quad_policy_act with epilogue + quad_step, then quad_rollout_post) with cursor t = t0.
 * Requires: a handle with env_kind HOVER or TRAJ, wrapper NONE or CTBR, auto_reset = 1.
 * Step t (t0 <= t < t0 + steps) writes row t % rows of the time-major buffers (every row pointer
 * required) and draws its action noise from Philox(seed; env_id_base + env, t, 0x200).
 * last_obs / last_start / ep_ret / ep_len carry the rollout across calls (read at entry, written
 * at exit); stats[slot] accumulate (finished return, length, count) as in QuadRolloutPost. */
typedef struct QuadRollout {
  float* obs_copy;          /* [rows,N,12] observation the step's action was taken from */
  float* actions;           /* [rows,N,4] unclipped sample (16-byte aligned) */
  float* log_prob;          /* [rows,N] */
  float* value;             /* [rows,N] V(obs) */
  float* episode_starts;    /* [rows,N] */
  float* rewards;           /* [rows,N] reward (+ gamma V(terminal_obs) on time-limit truncation) */
  float* last_obs;          /* [N,12] in: obs of step t0; out: obs after the last step */
  float* last_start;        /* [N] in/out: 1.0 where the next step begins an episode */
  float* ep_ret;            /* [N] in/out: running episode return */
  float* ep_len;            /* [N] in/out: running episode length */
  double* stats;            /* [QUAD_POLICY_STAT_SLOTS][3], accumulated */
  int32_t rows;             /* >= 1 */
  int32_t t0;               /* >= 0 */
  int32_t steps;            /* >= 1 */
  int32_t deterministic;    /* 1: a = mean */
  uint64_t seed;            /* action-noise seed */
  float gamma;
} QuadRollout;
int quad_rollout(QuadHandle* h, const float* packed, const QuadRollout* r, void* stream);

/* ---- PPO minibatch gradient on MFMA (row P): the gradient of SB3 PPO.train's minibatch loss
 * (stable_baselines3 ppo.py, as train.py:50-68 configures it; ppo/ppo.py ppo_loss restates it)
 *   loss = -mean(min(A r, A clip(r, 1 - clip_range, 1 + clip_range)))
 *          + ent_coef * (-entropy) + vf_coef * mean((returns - V)^2),
 *   r = exp(log_prob(actions) - old_log_prob), A = (adv - mean(adv)) / (std(adv) + 1e-8) over the
 *   minibatch (unbiased std; skipped when normalize_advantage == 0 or batch == 1),
 * with respect to every policy parameter, for the ActorCritic of QuadPolicyParams. Rows of the
 * flattened rollout buffer are gathered through `index` (a slice of the epoch's permutation), so
 * no minibatch copy is made. Ties of the min and the clip bounds follow torch's autograd
 * (torch.min splits a tie's gradient in half; clamp passes it on the closed interval). Gradients
 * are OVERWRITTEN (not accumulated) into `grads` (same shapes as the parameters); nothing in the
 * launch sequence synchronizes the host, so it is graph-capturable. */
typedef struct QuadPolicyGrads {
  float *pi_w0, *pi_b0, *pi_w1, *pi_b1, *act_w, *act_b;
  float *vf_w0, *vf_b0, *vf_w1, *vf_b1, *val_w, *val_b;
  float* log_std;
} QuadPolicyGrads;

typedef struct QuadPPOBatch {
  const float* obs;         /* [M,12] rollout buffer rows (16-byte aligned) */
  const float* actions;     /* [M,4] unclipped actions (16-byte aligned) */
  const float* log_prob;    /* [M] old log-probabilities */
  const float* advantages;  /* [M] */
  const float* returns;     /* [M] */
  const int64_t* index;     /* [batch] rows of this minibatch, each in [0, M) */
  int32_t batch;            /* >= 1 */
  int32_t normalize_advantage;  /* 0: off; 1: on; QUAD_ADV_PRECOMPUTED: on, and quad_ppo_adv_stats already
                                   wrote this minibatch's sums into the same workspace (stream-ordered);
                                   QUAD_ADV_GIVEN: on, with the sums in adv_sums */
  float clip_range, ent_coef, vf_coef;
  float* stats;             /* [4] out, or NULL: pg_loss, vf_loss, entropy, clip_fraction */
  const double* adv_sums;   /* QUAD_ADV_GIVEN: this minibatch's [QUAD_ADV_SUM_DOUBLES] block sums (a slice of
                               quad_ppo_adv_stats_epoch's output); ignored otherwise (ABI v5) */
} QuadPPOBatch;

/* ---- The optimizer step of PPO.train (row P), fused: torch.nn.utils.clip_grad_norm_(params,
 * max_grad_norm) followed by torch.optim.Adam.step() (SB3's policy optimizer, eps = 1e-5 in
 * train.py's policy_kwargs) over up to QUAD_ADAM_MAX_TENSORS device fp32 tensors, in two launches:
 *   total = ||all grads||_2; coef = min(max_grad_norm / (total + 1e-6), 1); grad *= coef
 *   (skipped when max_grad_norm <= 0); step += 1; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).
 * `step` points at each tensor's step counter (torch's float32 state["step"]); all are incremented. */
enum { QUAD_ADAM_MAX_TENSORS = 16 };
typedef struct QuadAdam {
  float* params[QUAD_ADAM_MAX_TENSORS];
  float* grads[QUAD_ADAM_MAX_TENSORS];       /* clipped in place, as clip_grad_norm_ does */
  float* exp_avg[QUAD_ADAM_MAX_TENSORS];
  float* exp_avg_sq[QUAD_ADAM_MAX_TENSORS];
  float* step[QUAD_ADAM_MAX_TENSORS];
  int32_t numel[QUAD_ADAM_MAX_TENSORS];
  int32_t count;                             /* tensors in use, 1..QUAD_ADAM_MAX_TENSORS */
  float max_grad_norm;
  double lr, beta1, beta2, eps;              /* moments and step size are formed in float64 */
} QuadAdam;
/* Device workspace (bytes) quad_clip_adam needs (gradient-norm partials). */
int64_t quad_adam_workspace_bytes(const QuadAdam* a);
int quad_clip_adam(const QuadAdam* a, void* workspace, int64_t workspace_bytes, void* stream);

/* The epoch permutation of PPO.train (SB3: np.random.permutation(buffer_size), the minibatch
 * index source of train.py:50-68's learner): out[i], i < n, is a permutation of [0, n) keyed by
 * `seed` -- a 4-round Feistel bijection of [0, 4^k) (4^k < 4n) restricted to [0, n) by cycle
 * walking. Device int64 [n]; n in [1, 2^40]. */
int quad_permutation(int64_t n, uint64_t seed, int64_t* out, void* stream);

/* Device workspace (bytes) quad_ppo_grad needs for a minibatch of `batch` rows. */
int64_t quad_ppo_workspace_bytes(int32_t batch);
/* Which kernel quad_ppo_grad launches: 1 = k_ppo_grad_x3 (bf16 MFMA on three-piece splits of every
 * f32 operand, f32-level error; the default), 0 = k_ppo_grad (f32-input MFMA; environment
 * QUADENV_LEARNER=f32, read on every call). Both meet the same accuracy bar. A captured update
 * (ppo.py graph_update, the default) replays the launches of the form -- and of the
 * QUADENV_LEARNER_SPLIT setting -- active at capture; a later change takes effect at the next capture. */
int quad_ppo_grad_form(void);
int quad_ppo_grad(const QuadPolicyParams* params, const QuadPPOBatch* b, const QuadPolicyGrads* grads,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* The minibatch advantage statistics quad_ppo_grad's normalization needs (sum, sum of squares,
 * float64), on their own: a data-parallel learner enqueues them for the NEXT minibatch while the
 * gradient all-reduce of this one is in flight (they read only advantages[index]), then calls
 * quad_ppo_grad with normalize_advantage = QUAD_ADV_PRECOMPUTED and the same workspace. */
enum { QUAD_ADV_PRECOMPUTED = 2, QUAD_ADV_GIVEN = 3 };
int quad_ppo_adv_stats(const QuadPPOBatch* b, void* workspace, int64_t workspace_bytes, void* stream);
/* The same statistics for every minibatch of an epoch in ONE launch (SB3 PPO.train normalizes each
 * minibatch by its own mean / std; minibatch m is rows perm[m * batch .. (m + 1) * batch) of the
 * epoch permutation): sums[m * QUAD_ADV_SUM_DOUBLES ...] receives minibatch m's block sums in the
 * fixed order quad_ppo_adv_stats uses, so quad_ppo_grad with normalize_advantage = QUAD_ADV_GIVEN and
 * adv_sums = that slice gives bit-identical gradients. One full-occupancy launch per epoch instead
 * of n_minibatches latency-bound 256-block pre-passes. */
#define QUAD_ADV_SUM_DOUBLES 512
int quad_ppo_adv_stats_epoch(const float* advantages, const int64_t* perm, int32_t batch, int32_t n_minibatches,
                             double* sums, void* stream);
/* ---- The same minibatch gradient for the general actor's family: policy net 12 -> h1 -> h2 -> 4 and
 * value net 12 -> h1 -> h2 -> 1 of the same widths (ActorCritic's MlpExtractor), h1 a multiple of 32 in [32, 512],
 * h2 in {64, 128, 256}, QUAD_ACTFN_RELU or QUAD_ACTFN_TANH. QuadPolicyParams / QuadPolicyGrads as above with the
 * arch's shapes (torch's [out, in]): pi_w0, vf_w0 [h1,12]; pi_w1, vf_w1 [h2,h1]; act_w [4,h2]; val_w [1,h2].
 * Semantics are quad_ppo_grad's: the SB3 loss, the unbiased advantage std (skipped at batch == 1), torch's tie rule
 * for the min and the closed clamp interval, the state-independent log_std gradient and entropy, stats[4], gradients
 * overwritten, rows gathered through `index`, no host synchronisation (graph-capturable). The gradient is
 * bit-identical from run to run and under a physical reordering of the rows into index order (no atomics; every sum
 * runs over the minibatch positions in a fixed order). normalize_advantage: 0, 1 (own pre-pass) or QUAD_ADV_GIVEN
 * (adv_sums from quad_ppo_adv_stats_epoch: the same bits as 1); QUAD_ADV_PRECOMPUTED belongs to quad_ppo_grad's
 * workspace layout and is QUAD_EINVAL here. batch in [1, 2^22]; the workspace holds the hidden images of every row
 * (about 8 (2 h1 + h2) bytes per row). tanh is the forward kernels' (quad_actor_act). QUAD_EINVAL with nothing
 * launched and nothing written: an arch outside the family (quad_ppo_arch_workspace_bytes: 0), NULL or misaligned
 * pointers (4 bytes; obs, actions, workspace 16; index, adv_sums 8), batch < 1, a workspace that is too small,
 * clip_range <= 0. The 12-128-128 ReLU net is a member; quad_ppo_grad keeps its own kernels for it.
 * The added entry points did not change the ABI version. */
int64_t quad_ppo_arch_workspace_bytes(const QuadActorArch* arch, int32_t batch);
int quad_ppo_arch_grad(const QuadActorArch* arch, const QuadPolicyParams* params, const QuadPPOBatch* b,
                       const QuadPolicyGrads* grads, void* workspace, int64_t workspace_bytes, void* stream);
/* Diagnostics (parity tests): quad_ppo_grad through a build of the same kernel body that also
 * records the hidden pre-activations (before the ReLU) it computed for every minibatch row:
 * hidden[(net * batch + pos) * 256 + 128 * layer + neuron], net 0 = actor / 1 = critic, pos = the
 * row's position in `index`, layer 0 = h1 / 1 = h2 (device float32 [2][batch][256]). The gradients
 * are written as by quad_ppo_grad. Lets a test count the kernel's own ReLU decisions against
 * float64 (no reference interface: SB3 exposes no such hook). */
int quad_ppo_hidden(const QuadPolicyParams* params, const QuadPPOBatch* b, const QuadPolicyGrads* grads,
                    float* hidden, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The rollout of the general actor's family: quad_policy_pack / quad_policy_act / quad_rollout_post /
 * quad_rollout for a policy net 12 -> h1 -> h2 -> 4 and a value net 12 -> h1 -> h2 -> 1 of the same widths and
 * activation (QuadPolicyParams with the arch's shapes, as quad_ppo_arch_grad reads it), on quad_actor_act's forward.
 * The packed image is quad_actor_pack's image of the policy net (to the bit), then the value net's image in the same
 * layout (a head of four outputs whose rows 1..3 are zero), then log_std[4]: 2 quad_actor_packed_floats + 4 floats.
 *   quad_actor_critic_act   quad_policy_act's semantics for QuadPolicyAct, field for field: the draw
 *                           Philox(seed; env_id_base + env, t, 0x200) + Box-Muller, a = mean + exp(log_std) z, the
 *                           log-prob recomputed from the stored a, actions_env = clip(a), every row pointer optional,
 *                           the cursor protocol, the fused epilogue of step t-1, deterministic. The mean is
 *                           quad_actor_act's, bit for bit.
 *   quad_actor_critic_post  quad_rollout_post.
 *   quad_actor_rollout      quad_rollout for QuadRollout: a handle with env_kind HOVER or TRAJ, wrapper NONE or CTBR,
 *                           auto_reset = 1; every row pointer required; last_obs / last_start / ep_ret / ep_len carried
 *                           across calls, stats accumulated; bit-identical to quad_actor_critic_act with the epilogue
 *                           + quad_step per step, then quad_actor_critic_post, with cursor t = t0.
 * QUAD_EINVAL with nothing launched and nothing written: an arch outside the family
 * (quad_actor_critic_packed_floats: < 0), a handle of another kind or wrapper, auto_reset = 0, rows < 1, steps < 1,
 * t0 < 0, a NULL required pointer, packed / actions / obs_copy / last_obs not 16-byte aligned.
 * The added entry points did not change the ABI version. */
int64_t quad_actor_critic_packed_floats(const QuadActorArch* arch);
int quad_actor_critic_pack(const QuadActorArch* arch, const QuadPolicyParams* p, float* packed, void* stream);
int quad_actor_critic_act(const QuadActorArch* arch, const float* packed, const QuadPolicyAct* a, int32_t n,
                          void* stream);
int quad_actor_critic_post(const QuadActorArch* arch, const float* packed, const QuadRolloutPost* p, uint32_t* cursor,
                           int32_t n, void* stream);
int quad_actor_rollout(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadRollout* r,
                       void* stream);

/* ---- quad_actor_rollout on the deployed observation: the policy is trained on what policy_node.py will
 * hand it -- the velocity of QuadVelEst's low-pass on finite differences of the position, the normalised vector
 * clipped to [-1, 1]. quad_actor_rollout's requirements and buffers; est->state (float64 [8][N], required) is read at
 * entry and written at exit, est->alpha may be NULL (alpha_all), the timestamp of step count k is k * est_dt.
 * Per env and step: both nets act on the deployed row in hand, which goes to obs_copy (sample, log-prob, clip and
 * the stored rows as in quad_actor_rollout); the env step, unchanged; one estimator update on the step's state12
 * position at (the env's step count after the step) * est_dt, and deploy_obs with the target the step's own
 * observation was built with: row D. On a time-limit truncation the bootstrap is gamma * V(D). An env that finished
 * is auto-reset as in quad_actor_rollout; its estimator is emptied (eight zeros) and updated once with the reset
 * state's position at (the reset step count) * est_dt, and the next row in hand is deploy_obs of the reset state, as
 * quad_observe reports it, with the new target (velocity 0); an env that did not finish carries D. At exit last_obs holds the row in hand and
 * est->state the estimators, so a rollout split over several calls gives the bits of one call.
 * Contract: bit-identical to this loop on a second handle, with cursor t = t0: per step quad_actor_critic_act, its
 * epilogue reading a terminal_obs buffer that holds D; quad_step; quad_deploy_obs_rows (rows NULL, timestamps the
 * new step counts * est_dt) on the step's state12 and the pre-reset target, D written to that buffer and to
 * last_obs; quad_observe with state12, then quad_deploy_obs_rows into last_obs with code 2 on the rows that
 * finished and 0 elsewhere (the handle's new target, timestamps the reset step counts * est_dt); and
 * quad_actor_critic_post at the end.
 * QUAD_EINVAL with nothing launched and nothing written: everything quad_actor_rollout refuses; a NULL est, a NULL
 * est->state or one that is not 8-byte aligned; QuadVelEst's own checks (alpha_all, max_dt); est_dt <= 0 or not
 * finite. quad_rollout (the 128-128 ReLU kernel, at its register limit) has no deployed form: the family's
 * (128, 128) ReLU instance collects that net. The population form is quad_pop_create_deployed (below). The added
 * entry points did not change the ABI version. */
int quad_actor_rollout_deployed(QuadHandle* h, const QuadActorArch* arch, const float* packed, const QuadRollout* r,
                                const QuadVelEst* est, double est_dt, void* stream);

/* ---- PPO populations in lock-step launches (added within ABI v8, whose number an
 * existing layout test pins: a v8 library built before these entry points lacks the quad_pop_* exports, and the
 * Python binding says so when it loads one): P independent small learners that share
 * every shape -- env kind, wrapper and constants, envs per member N, rollout rows T, minibatch size B -- and
 * differ in their pointers, seeds and scalar hyperparameters. Each call below does, in ONE launch per kernel
 * family, what P single calls do (the member is one more grid dimension; its block reads the member's
 * argument struct from a device table and runs the single kernel's body), so member m's outputs are
 * bit-identical to the single calls on member m's arguments.
 *   quad_pop_pack            quad_policy_pack(params -> packed)
 *   quad_pop_rollout         quad_rollout(env, packed, rollout with the given t0 / steps)
 *   quad_pop_value           quad_policy_act(deterministic, rows = 1): V(rollout.last_obs) -> last_values
 *   quad_pop_gae             quad_gae(rollout buffers, last_values, rollout.last_start, rollout.gamma, gae_lambda)
 *   quad_pop_permutation     quad_permutation(T N, seeds[m]) -> perm
 *   quad_pop_adv_stats_epoch quad_ppo_adv_stats_epoch(advantages, perm, B, T N / B) -> adv_sums
 *   quad_pop_ppo_grad        quad_ppo_grad (bf16x3 form) on minibatch `slot` of the epoch: index = perm + slot B,
 *                            adv_sums row `slot` (QUAD_ADV_GIVEN), stats -> mb_stats + 4 slot
 *   quad_pop_clip_adam       quad_clip_adam(adam)
 * The tables are built once by quad_pop_create (which validates every member and copies the tables to the
 * device; it synchronizes) and reused: a launch call makes no allocation, no host-to-device copy and no host
 * synchronization, so every launch call is stream-ordered and graph-capturable. A launch covers a SUBSET of
 * the members: quad_pop_subset registers a list of distinct member indices once (one small upload) and
 * returns its id; id 0 is every member. Members outside the subset are not touched. The member's buffers
 * are referenced, not copied: keep them alive and in place for the lifetime of the population. A table entry
 * also holds the env handle's parameters as they are at creation (its seed among them): do not quad_seed a
 * member's handle afterwards. */
typedef struct QuadPopMember {
  QuadHandle* env;          /* the member's own env handle (quad_rollout's requirements) */
  QuadPolicyParams params;
  QuadPolicyGrads grads;
  QuadAdam adam;            /* with the member's lr, betas, eps, max_grad_norm */
  float* packed;            /* [quad_policy_packed_floats()] (16-byte aligned) */
  QuadRollout rollout;      /* the member's buffers, rows = T, seed, gamma; t0 and steps are given per launch */
  float* last_values;       /* [N] V(last_obs), written by quad_pop_value */
  float* scratch_actions;   /* [N,4] the deterministic actions quad_pop_value also writes */
  float* advantages;        /* [T,N] */
  float* returns;           /* [T,N] */
  int64_t* perm;            /* [T N] the epoch permutation */
  double* adv_sums;         /* [T N / B][QUAD_ADV_SUM_DOUBLES] */
  float* mb_stats;          /* [T N / B][4]: pg_loss, vf_loss, entropy, clip_fraction per minibatch slot */
  void* workspace;          /* quad_pop_workspace_bytes(adam, B) bytes, 16-byte aligned */
  int64_t workspace_bytes;
  float gae_lambda, clip_range, ent_coef, vf_coef;
} QuadPopMember;
typedef struct QuadPop QuadPop;
/* Device workspace (bytes) one member needs: gradient partials, the W2 image, the gradient-norm partials.
 * 0 on invalid arguments. */
int64_t quad_pop_workspace_bytes(const QuadAdam* adam, int32_t batch);
/* QUAD_EINVAL (nothing allocated, *out = NULL) for: P < 1 or P > 65,535; a NULL required pointer; a misaligned buffer;
 * members whose shapes (env kind, wrapper, constants, N, rows, Adam tensor sizes) differ; an env kind or
 * wrapper quad_rollout rejects; batch < 1 or > 8192 (the separate-block gradient form's limit); T N not a
 * multiple of batch; a workspace that is too small; hyperparameters quad_ppo_grad / quad_clip_adam reject;
 * QUADENV_LEARNER=f32 (only the bf16x3 gradient has a population form). */
int quad_pop_create(const QuadPopMember* members, int32_t P, int32_t batch, int32_t normalize_advantage,
                    QuadPop** out);
void quad_pop_destroy(QuadPop* pop);
/* Register the subset `members[0..count)` (distinct indices in [0, P)); *subset_id receives its id.
 * QUAD_EINVAL for an empty list, an index out of range or a duplicate. */
int quad_pop_subset(QuadPop* pop, const int32_t* members, int32_t count, int32_t* subset_id);
int quad_pop_pack(QuadPop* pop, int32_t subset, void* stream);
int quad_pop_rollout(QuadPop* pop, int32_t subset, int32_t t0, int32_t steps, void* stream);
int quad_pop_value(QuadPop* pop, int32_t subset, void* stream);
int quad_pop_gae(QuadPop* pop, int32_t subset, void* stream);
/* seeds: device uint64 [P], indexed by MEMBER (entries of members outside the subset are not read) */
int quad_pop_permutation(QuadPop* pop, int32_t subset, const uint64_t* seeds, void* stream);
int quad_pop_adv_stats_epoch(QuadPop* pop, int32_t subset, void* stream);
int quad_pop_ppo_grad(QuadPop* pop, int32_t subset, int32_t slot, void* stream);
int quad_pop_clip_adam(QuadPop* pop, int32_t subset, void* stream);

/* Evaluation episodes of a population in ONE launch: quad_policy_episode (env-observation mode) for every
 * member of the subset on an evaluation handle of the member's own and the member's packed image
 * (quad_pop_pack first, after an update). quad_pop_attach_eval validates evals[0..P) -- one per member, each
 * what quad_policy_episode takes; env = NULL for a member that is not evaluated -- builds the table and uploads
 * it once; calling it again replaces the table. The table holds each handle's parameters (its seed among them)
 * as they are when attached and refers to the handle's state: quad_pop_detach_eval before an evaluation handle
 * is destroyed or re-seeded (quad_pop_episode then returns QUAD_EINVAL until the next attach). quad_pop_episode
 * also rejects a subset with a member that has no handle attached.
 * QUAD_EINVAL for anything quad_policy_episode rejects, obs_mode != QUAD_OBS_ENV, and evaluation handles whose
 * env kind, wrapper, constants or env count differ, or run.max_steps that differ. Every env of every member
 * flies from its current state (reset the handles first) to its first terminated / truncated step or
 * max_steps and is frozen; each member's metrics arrays are written as quad_policy_episode writes them. */
typedef struct QuadPopEval {
  QuadHandle* env;          /* the member's evaluation handle (any auto_reset setting) */
  QuadPolicyRun run;        /* obs_mode QUAD_OBS_ENV; the member's own metrics / trace / estimator arrays */
} QuadPopEval;
int quad_pop_attach_eval(QuadPop* pop, const QuadPopEval* evals);
int quad_pop_detach_eval(QuadPop* pop);
int quad_pop_episode(QuadPop* pop, int32_t subset, void* stream);

/* ---- Populations of the general actor's family (added within ABI v8 as the entry points above were):
 * the same QuadPop, QuadPopMember and launch calls for P learners that share one QuadActorArch -- policy net
 * 12 -> h1 -> h2 -> 4 and value net 12 -> h1 -> h2 -> 1, h1 a multiple of 32 up to 512, h2 in {64, 128, 256}, ReLU or
 * tanh. A member's params / grads are read with the arch's shapes and its packed image holds
 * quad_actor_critic_packed_floats(arch) floats. On such a population
 *   quad_pop_pack            is quad_actor_critic_pack(arch, params -> packed)
 *   quad_pop_rollout         is quad_actor_rollout(env, arch, packed, rollout with the given t0 / steps); block b of a
 *                            member's launch holds 64 envs and adds its episode statistics into
 *                            rollout.stats[b % QUAD_POLICY_STAT_SLOTS]: with more than 64 envs sum the slots
 *   quad_pop_value           is quad_actor_critic_act(deterministic, rows = 1): V(rollout.last_obs) -> last_values
 *   quad_pop_ppo_grad        is quad_ppo_arch_grad with QUAD_ADV_GIVEN on minibatch `slot` of the epoch
 *   quad_pop_attach_eval / quad_pop_episode are quad_actor_episode (env-observation mode) on the policy half of the
 *                            member's image (its first quad_actor_packed_floats(arch) floats)
 * and quad_pop_gae / _permutation / _adv_stats_epoch / _clip_adam / _subset / _detach_eval / _destroy are what they
 * are above; every launch call stays free of allocations, copies and synchronization. */
/* Device workspace (bytes) one member needs: quad_ppo_arch_workspace_bytes(arch, batch), then the gradient-norm
 * partials. 0 on invalid arguments (an arch outside the family, batch < 1 or > 8192, an invalid QuadAdam). */
int64_t quad_pop_arch_workspace_bytes(const QuadActorArch* arch, const QuadAdam* adam, int32_t batch);
/* quad_pop_create for the family. QUAD_EINVAL (nothing allocated, nothing launched, *out = NULL) for an arch outside
 * the family, anything quad_pop_create rejects in a member (QUADENV_LEARNER aside), Adam tensors whose sizes are not
 * the 13 of the arch's module, and a workspace smaller than quad_pop_arch_workspace_bytes. */
int quad_pop_create_arch(const QuadActorArch* arch, const QuadPopMember* members, int32_t P, int32_t batch,
                         int32_t normalize_advantage, QuadPop** out);

/* ---- Populations trained on the deployed observation (added within ABI v8 as the entry points above
 * were, no existing struct changed): quad_pop_create_arch's QuadPop, QuadPopMember and launch calls for P learners of
 * one QuadActorArch whose rollouts are quad_actor_rollout_deployed's. deploy[m] is member m's estimator -- what
 * quad_actor_rollout_deployed takes: est.state float64 [8][N] required, read at the entry of a rollout launch and
 * written at its exit, referenced and not copied; est.alpha [N] or NULL for alpha_all -- and est_dt; members may
 * differ in alpha_all, in their alpha arrays and in max_dt. On such a population
 *   quad_pop_pack, quad_pop_value   are the family's (quad_actor_critic_pack / quad_actor_critic_act), as on a
 *                            quad_pop_create_arch population; packed holds quad_actor_critic_packed_floats(arch)
 *   quad_pop_rollout         is quad_actor_rollout_deployed(env, arch, packed, rollout with the given t0 / steps,
 *                            &deploy[m].est, deploy[m].est_dt): rollout.last_obs holds the deployed row in hand
 *   quad_pop_ppo_grad        is quad_ppo_arch_grad, as on a quad_pop_create_arch population -- except for the
 *                            (128, 128) ReLU arch: there it is quad_ppo_grad (bf16x3 form) as on a quad_pop_create
 *                            population, the pairing a single deployed learner of that net has, with the workspace
 *                            of quad_pop_workspace_bytes
 *   quad_pop_attach_eval     requires obs_mode == QUAD_OBS_DEPLOYED on every attached run (its estimator arguments
 *                            as quad_actor_episode takes them) and refuses QUAD_OBS_ENV; on every other population
 *                            it refuses QUAD_OBS_DEPLOYED, as before
 *   quad_pop_episode         is quad_actor_episode in deployed mode on the policy half of the member's image
 * and quad_pop_gae / _permutation / _adv_stats_epoch / _clip_adam / _subset / _detach_eval / _destroy are what they are
 * above. Launch calls stay free of allocations, copies and synchronization. */
typedef struct QuadPopDeploy {
  QuadVelEst est;
  double est_dt;            /* the timestamp of step count k is k * est_dt (the env's dt) */
} QuadPopDeploy;            /* one per member */
/* Device workspace (bytes) one member needs: quad_pop_workspace_bytes(adam, batch) for the (128, 128) ReLU arch,
 * quad_pop_arch_workspace_bytes(arch, adam, batch) for every other arch of the family. 0 on invalid arguments. */
int64_t quad_pop_deployed_workspace_bytes(const QuadActorArch* arch, const QuadAdam* adam, int32_t batch);
/* QUAD_EINVAL (nothing allocated, nothing launched, *out = NULL) for everything quad_pop_create_arch rejects (the
 * (128, 128) ReLU arch is accepted here; for it also QUADENV_LEARNER=f32, as quad_pop_create), a NULL deploy, and per
 * member: a NULL est.state or one that is not 8-byte aligned, an est.alpha that is not 8-byte aligned, QuadVelEst's
 * own checks (alpha_all finite when alpha is NULL, max_dt > 0), est_dt <= 0 or not finite. */
int quad_pop_create_deployed(const QuadActorArch* arch, const QuadPopMember* members, const QuadPopDeploy* deploy,
                             int32_t P, int32_t batch, int32_t normalize_advantage, QuadPop** out);

#ifdef __cplusplus
}
#endif
#endif /* QUADENV_H */
