/*
 * hgym.h -- C-ABI of libhgym_hip.so: the MI355X (gfx950) hot path of roboterax/humanoid-gym.
 *
 * The reference (pure Python/PyTorch) has no FFI of its own; its replaceable seam is the Python API
 * of humanoid.envs / humanoid.algo.ppo.  Each entry point below states the reference
 * interface (file:line under /root/reference/humanoid) it stands in for.  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 (HGYM_OK) or a negative HGYM_E_* code; hgym_last_error() gives the
 *     thread-local message of the last failure.
 *   - the CALLER owns every buffer (PyTorch allocates them); the library never allocates or frees
 *     device memory and keeps no pointer past the call.
 *   - all device work is enqueued on the hipStream_t passed as `void* stream`; no call synchronises,
 *     all calls are hipGraph-capturable, and per-step counters live in device memory so that a
 *     replayed graph advances them.
 *   - plain pointers and sizes only: no torch types cross this boundary.
 *   - per-env state is env-major SoA: a field with C components is a [C][N] fp32 array, so that
 *     lane i of a wavefront touches env i of every component (coalesced).  The (N,C) tensors of the
 *     reference API are transposed views of these arrays.
 */
#ifndef HGYM_H_
#define HGYM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGYM_VERSION 9      /* 2: HgymEnvOut carries the logging sink; hgym_rollout_*, hgym_ppo_grad_part, hgym_net_param_offset
                             * 3: the rollout scratch block grows with the env count (HGYM_ROLLOUT_SCRATCH_BYTES(num_envs))
                             * 4: bf16 observation shadow: HgymObsShadow argument of the policy launches, HgymBatch.obs_bf16 /
                             *    priv_bf16, hgym_net_shadow_ld
                             * 5: HgymEnvOut.obs_ahead / obs_older_ready (hgym_rollout_step writes the older frames one launch ahead)
                             * 6: HgymEnvOut.l0_ahead / l0_ready / obs_bf16_ahead (the actor's first layer carried across the launches of a rollout);
                             *    HGYM_MAX_CUSTOM_REWARDS 8 -> 24, custom_reward_pos = 23: after the clip (`termination`);
                             *    (same version, later: frames written into obs_ahead / priv_ahead for an env that resets in the same step are
                             *    zeroed by the NEXT hgym_rollout_step call -- see HgymEnvOut.obs_ahead; layouts and call sequence unchanged)
                             * 7: HgymComm.wait_ticks (bound of the direct exchange's waits) + hgym_comm_status; a communicator stays usable
                             *    after an expired wait (the done counter is per call); HgymEnvOut.t_time_outs, hgym_critic_values,
                             *    hgym_gae_bootstrap and hgym_rollout_step with values = NULL (the critic run once after the rollout)
                             * 8: hgym_gae / hgym_gae_bootstrap: `stats` is HGYM_GAE_STATS_DOUBLES(n) doubles (per-workgroup partial sums + arrival
                             *    counter behind the three results), the advantage statistics are summed in a fixed order
                             * 9: hgym_randperm_dev (draw number on the device); hgym_comm_allreduce(seq = 0): the call number kept on the device
                             *    (status[2]); hgym_comm_sum64 -- what a captured update needs: no launch argument changes between iterations
                             *    (same version, later: HgymNetConfig.activation / act_alpha / act_scale appended -- ELU, SELU, LeakyReLU / ReLU,
                             *    Tanh or Sigmoid between the Linear layers; a zero-filled tail is the ELU(1) every earlier layout meant)
                             *    (same version, later still: HgymPPOConfig.value_loss_unclipped appended -- the value loss (R - V)^2 instead of
                             *    the clipped form; a zero-filled tail is the clipped loss every earlier layout meant)
                             *    (same version, later: HgymNetConfig.fused_activation appended -- the fused bf16 forward / update kernels for
                             *    every activation instead of ELU(1) only; a zero-filled tail is the ELU(1)-only rule every earlier layout meant)
                             *    (same version, later: hgym_env_reset_idx -- reset_idx for a caller-chosen subset of envs, its draws keyed by
                             *    the call number in HgymEnvState.counters[HGYM_CNT_RESET_CALL]; no layout changes)
                             *    (same version, later: hgym_rollout_eval_step -- the rollout launch on the policy's mean action -- and the
                             *    evaluation accumulator hgym_eval_reset / hgym_eval_accumulate; no layout changes)
                             *    (same version, later: the diagnostics pass behind an update -- hgym_ppo_diag_reset, hgym_ppo_diag_reduce,
                             *    hgym_ppo_diagnostics; no layout changes)
                             *    (same version, later: names for the slots of opt_state, log_stats and counters -- HGYM_OPT_*, HGYM_LOG_*,
                             *    HGYM_CNT_*; no layout changes)
                             *    (same version, later: HgymNetConfig.std_param added ahead of fused_activation -- the action noise trained as log sigma
                             *    (HGYM_STD_LOG) -- and hgym_net_sigma_offset; a zero-filled field is the sigma parameter every earlier layout meant)
                             *    (same version, later: hgym_mirror_rows -- the mirrored copy of stored rows for left-right symmetry augmentation;
                             *    no layout changes)
                             *    (same version, later: HgymNet.norm appended -- empirical observation normalisation folded into the first layer,
                             *    hgym_net_norm_*; a NULL (zero-filled) member is a net without it)
                             *    (same version, later: HgymPPOConfig.mirror_coef and HgymBatch.pair_idx / mirror_act_src / mirror_act_sign /
                             *    mirror_target / mirror_sums appended -- the mirror loss of left-right symmetry; a zero-filled tail is off)
                             *    (same version, later: hgym_adv_normalize_minibatches -- advantages standardised per minibatch into a second column;
                             *    no layout changes)
                             *    (same version, later: hgym_bc_grad and HgymBCConfig -- one behaviour-cloning minibatch of the actor, rsl_rl's
                             *    Distillation; no layout changes)
                             *    (same version, later: hgym_rnd_block_init, hgym_rnd_rewards and HgymRndConfig -- Random Network Distillation's
                             *    reward pass; no layout changes)
                             *    (same version, later: hgym_smooth_pairs, hgym_perturb_rows, hgym_ppo_grad_smooth and HgymSmooth -- the smoothness
                             *    regulariser on the policy's mean; no layout changes)
                             *    (same version, later: hgym_value_denormalize, hgym_value_norm_merge, hgym_value_normalize -- value targets
                             *    standardised by running statistics; no layout changes)
                             *    (same version, later: hgym_ppo_grad_smooth_mirror -- the mirror loss and the smoothness regulariser in one
                             *    actor head; no layout changes)
                             *    (same version, later: hgym_guide_schedule, hgym_ppo_grad_guide, HgymGuideSchedule and HgymGuide -- a frozen
                             *    teacher's cloning term with a device-resident coefficient; no layout changes)
                             *    (same version, later: hgym_vf_grad, hgym_bc_vf_grad and HgymVFConfig -- one minibatch of the critic alone, and
                             *    a cloning minibatch that also trains the critic; no layout changes) */

enum {
    HGYM_OK = 0,
    HGYM_E_BADARG = -1,      /* null pointer, negative size ... */
    HGYM_E_SHAPE = -2,       /* sizes inconsistent with the configuration */
    HGYM_E_LAUNCH = -3,      /* HIP reported an error at launch */
    HGYM_E_UNSUPPORTED = -4, /* configuration outside what the kernels were built for */
    HGYM_E_NODEVICE = -5     /* no gfx950 device visible */
};

#define HGYM_NUM_DOF 12
#define HGYM_NUM_ACTIONS 12
#define HGYM_NUM_BODIES 13
#define HGYM_NUM_REWARDS 22
#define HGYM_OBS_FRAME 47   /* num_single_obs,           envs/custom/humanoid_config.py:41 */
#define HGYM_PRIV_FRAME 73  /* single_num_privileged_obs, envs/custom/humanoid_config.py:43 */
#define HGYM_MAX_LAYERS 8
#define HGYM_MAX_CUSTOM_REWARDS 24  /* user-defined reward terms per env (HgymEnvConfig.num_custom_rewards): room for a task class that
                                      * defines every one of its terms itself, the reference's way */

int32_t hgym_version(void);
const char* hgym_last_error(void);
/* number of compute units of the current device (0 if none); also a cheap "is there a GPU" probe */
int32_t hgym_device_cus(void);
/* sizeof() of a struct of this header by name ("HgymEnvConfig", ...), -1 if unknown: lets a binding in
 * another language verify its mirror of the layouts */
int64_t hgym_sizeof(const char* name);

/* ------------------------------------------------------------------------------------------------
 * Env configuration = the constants of XBotLCfg the hot path reads
 * (envs/custom/humanoid_config.py:34-227, envs/base/legged_robot.py:710-720).
 * ---------------------------------------------------------------------------------------------- */
typedef struct HgymEnvConfig {
    int32_t num_envs;
    int32_t frame_stack;          /* 15 */
    int32_t c_frame_stack;        /* 3  */
    int32_t decimation;           /* 10 */
    float sim_dt;                 /* 0.001 */
    float dt;                     /* decimation*sim_dt as fp32(python double product) = 0.01f */
    int32_t max_episode_length;   /* 2400 */
    int32_t resample_steps;       /* 800 */
    int32_t push_interval;        /* 400 */
    int32_t push_robots;          /* 1 */
    int32_t add_noise;            /* 1 */
    int32_t heading_command;      /* 1 for XBot-L: the yaw-rate command follows a sampled heading (legged_robot.py:311-314); 0: the yaw
                                     rate itself is sampled from cmd_yaw_lo/span (:333-334) -- one of the generic options below */
    int32_t use_ref_actions;      /* 0 for XBot-L (humanoid_config.py:49); 1: actions += 2 * ref_dof_pos, IN PLACE, before the clip
                                     (humanoid_env.py:190-191) */
    float clip_actions, clip_obs; /* 18, 18 */
    float action_scale;           /* 0.25 */
    float action_delay, action_noise; /* 0.5, 0.02 */
    float noise_level;            /* 0.6 */
    float obs_noise[HGYM_OBS_FRAME];   /* noise_scale_vec, humanoid_env.py:166-186 */
    float scale_lin_vel, scale_ang_vel, scale_dof_pos, scale_dof_vel, scale_quat;
    /* torch_rand_float(lo,hi) = (hi-lo)*u + lo with (hi-lo) formed in python double: carry lo and the
       double-rounded span so the fp32 arithmetic is the reference's (legged_robot.py:328-331,367) */
    float cmd_x_lo, cmd_x_span, cmd_y_lo, cmd_y_span, cmd_h_lo, cmd_h_span;
    float dof_reset_lo, dof_reset_span;       /* -0.1, 0.2 */
    float push_vel_lo, push_vel_span;         /* -0.2, 0.4   humanoid_env.py:86-89 */
    float push_ang_lo, push_ang_span;         /* -0.4, 0.8   humanoid_env.py:92-93 */
    float p_gains[HGYM_NUM_DOF], d_gains[HGYM_NUM_DOF], torque_limits[HGYM_NUM_DOF];
    float default_dof_pos[HGYM_NUM_DOF];
    float dof_lower[HGYM_NUM_DOF], dof_upper[HGYM_NUM_DOF]; /* synthetic physics only */
    float base_init_state[13];
    int32_t base_body, feet_bodies[2], knee_bodies[2];
    /* rewards (humanoid_config.py:174-216); scales already multiplied by dt, alphabetical order */
    float reward_scales[HGYM_NUM_REWARDS];
    int32_t only_positive_rewards;
    float base_height_target, min_dist, max_dist, target_joint_pos_scale, target_feet_height;
    float cycle_time, tracking_sigma, max_contact_force, episode_length_s;
    uint64_t seed;                /* Philox key for internally generated noise */
    /* ---- generic LeggedRobot options XBot-L leaves off.  All zero = plane terrain, fixed command
     * ranges: the XBot-L default, and the configuration the headline numbers are measured on. ---- */
    int32_t custom_origins;       /* terrain.mesh_type in {heightfield, trimesh} (legged_robot.py:687-697): a reset spawns the robot at
                                     its tile origin + U(-1,1) m in x and y (:382-385) */
    int32_t terrain_curriculum;   /* terrain.curriculum: on reset an env that walked more than half a tile is promoted one terrain
                                     level, one that covered less than half its commanded distance demoted; solving the last level
                                     redraws a random one (:176-177,400-420).  Needs custom_origins. */
    int32_t terrain_rows, terrain_cols;   /* levels x types of HgymEnvState.terrain_origins; max_terrain_level = terrain_rows (:695) */
    float terrain_env_length;     /* Terrain.env_length (utils/terrain.py:46) */
    int32_t num_height_points;    /* > 0: terrain.measure_heights with that many sample points per env (:316-317,743-795) */
    int32_t height_rows, height_cols;     /* shape of HgymEnvState.height_samples (Terrain.tot_rows, tot_cols) */
    float terrain_border, terrain_hscale, terrain_vscale;   /* terrain.border_size / horizontal_scale / vertical_scale */
    float cmd_yaw_lo, cmd_yaw_span;   /* commands.ranges.ang_vel_yaw, used when heading_command = 0 */
    int32_t command_curriculum;   /* commands.curriculum: every max_episode_length common steps, if the resetting envs' mean
                                     tracking_lin_vel episode sum exceeds 80 % of its maximum, lin_vel_x widens by 0.5 each way
                                     up to +-max_curriculum (:179-180,422-431).  The live range is HgymEnvState.command_range_x. */
    float max_curriculum;
    /* User-defined reward terms (legged_robot.py:518-541: every non-zero entry of cfg.rewards.scales names a method
     * `_reward_<name>`, found by name).  The 22 XBot-L terms are built in; any OTHER name is evaluated by the caller between
     * hgym_env_step_begin and hgym_env_step_end (what the reference has computed by the time compute_reward runs is then in the
     * state) and handed in through HgymEnvState.custom_rew.  custom_reward_pos[j] = how many built-in terms precede custom
     * term j in the alphabetical order the reference sums in (0 .. 22): the fp32 sum is formed in that merged order.
     * 23 (= HGYM_NUM_REWARDS + 1): the term is added AFTER the only_positive_rewards clip -- the reference's `termination`
     * (legged_robot.py:229-235; it is skipped in the function list, :533-534). */
    int32_t num_custom_rewards;
    int32_t custom_reward_pos[HGYM_MAX_CUSTOM_REWARDS];
} HgymEnvConfig;

/* fills *cfg with the XBot-L values (the reference defaults) for num_envs environments */
int32_t hgym_env_config_default(HgymEnvConfig* cfg, int32_t num_envs);

/* A strided view of one simulator tensor: element (env, comp) is base[env*env_stride + comp*comp_stride].
 * Isaac Gym's AoS buffers (legged_robot.py:449-457) and the library's own SoA synthetic backend are both
 * expressible.  comps: root 13 | dof_pos 12 | dof_vel 12 | contact body*3+axis (39) | rigid body*13+c (169). */
typedef struct HgymStrided {
    float* base;
    int64_t env_stride;
    int64_t comp_stride;
} HgymStrided;

typedef struct HgymSimTensors {
    HgymStrided root, dof_pos, dof_vel, contact, rigid;
} HgymSimTensors;

/* Per-env state, every field [C][N] fp32 SoA unless noted (legged_robot.py:434-516, base_task.py:71-94,
 * humanoid_env.py:78-79). */
typedef struct HgymEnvState {
    int64_t* episode_length;   /* [N] int64, VecEnv.episode_length_buf */
    int64_t* counters;         /* [4] int64 device scalars: [0] common_step_counter, [1] resets this step,
                                  [2] ring step (frames pushed so far), [3] host-reset call number: hgym_env_reset_idx
                                  keys its draws by it and advances it (zero-filled by the caller once; seek-style moves of
                                  [0] leave it alone) -- HGYM_CNT_* below */
    float* commands;           /* 4 */
    float* actions;            /* 12 */
    float* last_actions;       /* 12 */
    float* last_last_actions;  /* 12 */
    float* last_dof_vel;       /* 12 */
    float* last_root_vel;      /* 6 */
    float* torques;            /* 12 */
    float* feet_air_time;      /* 2 */
    float* last_contacts;      /* 2 (0/1) */
    float* feet_height;        /* 2 */
    float* last_feet_z;        /* 2 */
    float* ref_dof_pos;        /* 12 */
    float* push_force;         /* 3 */
    float* push_torque;        /* 3 */
    float* episode_sums;       /* 22 */
    float* base_lin_vel;       /* 3 */
    float* base_ang_vel;       /* 3 */
    float* projected_gravity;  /* 3 */
    float* base_euler;         /* 3 */
    float* friction;           /* 1 */
    float* body_mass;          /* 1 */
    float* env_origins;        /* 3 */
    float* obs_ring;           /* [N][frame_stack][47]   unclipped noisy frames, ring slot = ring step % frame_stack */
    float* priv_ring;          /* [N][c_frame_stack][73] */
    float* episode_acc;        /* [24] fp32 device scalars: sum over resetting envs of episode_sums[k]; [22] unused */
    /* generic options (HgymEnvConfig tail); NULL when the option is off */
    int64_t* terrain_levels;        /* (N,) int64  LeggedRobot.terrain_levels */
    const int64_t* terrain_types;   /* (N,) int64  LeggedRobot.terrain_types */
    const float* terrain_origins;   /* (terrain_rows, terrain_cols, 3) fp32 = Terrain.env_origins */
    const int16_t* height_samples;  /* (height_rows, height_cols) int16 = Terrain.heightsamples */
    const float* height_points;     /* (num_height_points, 3) base-frame sample points, the same for every env (:743-759) */
    float* height_pose;             /* (N, 7) scratch: base position + quaternion at the point of the step where the reference
                                       samples the heights (before the reset overwrites them) */
    float* measured_heights;        /* (N, num_height_points) fp32 = LeggedRobot.measured_heights */
    double* command_range_x;        /* [2] device doubles: command_ranges["lin_vel_x"] = [lo, hi]; moved by the command curriculum */
    /* user-defined reward terms (HgymEnvConfig.num_custom_rewards = K > 0; NULL otherwise) */
    const float* custom_rew;        /* (K, N) this step's terms, already times scale * dt: written by the caller between begin and end */
    float* custom_sums;             /* (K, N) their episode sums (episode_sums of the reference, legged_robot.py:225-227) */
    float* custom_acc;              /* (K,)   sum over the envs resetting this step of their episode sums (-> HgymEnvOut.extras_custom) */
} HgymEnvState;
/* slots of HgymEnvState.counters */
#define HGYM_CNT_STEP 0          /* common_step_counter */
#define HGYM_CNT_RESETS 1        /* resets this step */
#define HGYM_CNT_RING 2          /* ring step (frames pushed so far) */
#define HGYM_CNT_RESET_CALL 3    /* host-reset call number */

/* Outputs of one env step = the 5-tuple of VecEnv.step (algo/vec_env.py:50-51) plus the extras tensors. */
typedef struct HgymEnvOut {
    float* obs;                /* (N, frame_stack*47) row-major, clipped */
    float* priv_obs;           /* (N, c_frame_stack*73) row-major, clipped */
    float* rew;                /* (N,) */
    uint8_t* reset;            /* (N,) bool */
    uint8_t* time_out;         /* (N,) bool: this step's time_out_buf */
    uint8_t* extras_time_outs; /* (N,) bool: extras["time_outs"], refreshed only on steps with >=1 reset
                                  (legged_robot.py:173-174,209-210) */
    float* extras_episode;     /* (22,) extras["episode"]["rew_<term>"], same staleness rule */
    /* Optional transition sink (t_rewards == NULL: off).  When set, the step finaliser also does what
     * PPO.process_env_step + RolloutStorage.add_transitions do for the scalar columns (ppo.py:103-113,
     * rollout_storage.py:91-94; same arithmetic as hgym_store_step) from this step's rew / reset and the
     * just-refreshed extras["time_outs"], and bumps *t_step: one launch less per vec-step. */
    const float* t_values;     /* (N,) critic values of the transition being stored */
    float* t_rewards;          /* (N,) storage.rewards[step]  = rew + t_gamma * (values * extras_time_outs) */
    uint8_t* t_dones;          /* (N,) storage.dones[step]    = reset */
    int64_t* t_step;           /* device scalar += 1 per step (the policy's sampling-step counter), or NULL */
    float t_gamma;
    /* 1: the env-step entry points do NOT launch the step finaliser; the caller runs it before the next env step, either as
     * one extra workgroup of the next policy launch (hgym_policy_act_fin) or on its own (hgym_env_finalize).  *t_step is
     * then bumped by the env kernel itself.  Until the finaliser has run, the extras_* outputs, the transition-sink slots
     * and the step counters are those of the previous step. */
    int32_t defer_finalize;
    /* Optional logging sink (log_stats == NULL: off): the step finaliser also keeps OnPolicyRunner.learn's per-step book-keeping
     * (algo/ppo/on_policy_runner.py:143-156) on the device, so that a logging run needs no host work between vec-steps:
     *   log_cur   (2, N) fp32   cur_reward_sum | cur_episode_length of every env (+= rew, += 1; zeroed when the env is done)
     *   log_stats HGYM_LOG_STATS floats (HGYM_LOG_* below):
     *     [0, 22)    TERMS      sum over the steps since the caller last cleared it of extras["episode"][k] (what ep_infos.append collects)
     *     [22]       STEPS      number of those steps
     *     [24], [25] RING_HEAD, RING_FILL  head / fill count of the two rings below
     *     [32, 132)  RETURNS    returns of the last 100 (RING) finished episodes (rewbuffer, a deque(maxlen=100)), in env order within a step
     *     [132, 232) LENGTHS    their lengths (lenbuffer)
     * The caller zero-fills both once and clears log_stats[0, 23) = [0, HGYM_LOG_CLEAR) after reading it. */
    float* log_cur;
    float* log_stats;
    float* extras_custom;      /* (K,) extras["episode"]["rew_<name>"] of the user-defined terms, same staleness rule as extras_episode */
    /* hgym_rollout_step only (NULL / 0 everywhere else).  obs_ahead: rows of the observation AFTER `obs` ((N, frame_stack*47): the
     * rollout storage's slot after next).  The launch then also writes their frames 0 .. frame_stack-2 -- the frame_stack-2 older
     * frames it knows when it starts (copied by the tile's critic workgroup behind its tile) and this step's own frame -- so that
     * the NEXT launch, called with obs = this pointer and obs_older_ready = 1, does not copy them on its critical path: between the
     * first and second layer of the actor tile that copy costs 4.4 us of a 42 us launch.  The rows come out bit-identical.
     * For an env that resets in THIS step the copied frames are pre-reset history: the next call (obs_older_ready = 1, prev_out = this
     * call's out -- both already required) zeroes them before anybody reads the rows; a next call WITHOUT obs_older_ready writes all
     * older frames itself.  Do not read obs_ahead / priv_ahead rows between the two calls. */
    float* obs_ahead;
    float* priv_ahead;         /* the same for priv_obs ((N, c_frame_stack*73)); both or neither */
    int32_t obs_older_ready;   /* 1: frames 0 .. frame_stack-2 of `obs` (and 0 .. c_frame_stack-2 of `priv_obs`) were written by the
                                  previous launch (as its obs_ahead / priv_ahead) */
    /* hgym_rollout_step only, header v6 (NULL / 0 everywhere else): the actor's FIRST LAYER carried across launches.  The next row is
     * this row shifted by one frame plus the frame this step produces, so up to 20 of the first layer's 24 k-steps (columns [0, 640)
     * of the next row; 12 are taken by default) can be formed while this launch runs: its critic workgroups, idle for the second half of the launch, do that and
     * leave the fp32 partial pre-activations in l0_ahead ((num_envs, 512) floats, caller-owned, 16-byte aligned); the NEXT launch,
     * called with l0_ready = that buffer (and obs_older_ready = 1), starts its actor tile from them and reads only the remaining
     * columns of its rows.  Same fragments, same k order, same accumulator chain: bit-identical outputs.  Partial sums of rows whose
     * env was reset in between are dropped (their older frames are zero).  obs_bf16_ahead (optional, with l0_ahead): the bf16 shadow
     * rows of the NEXT step's observation (HgymObsShadow.obs of the next call): the columns formed ahead are written by this launch,
     * the next launch writes the rest and zeroes the former in reset rows. */
    float* l0_ahead;
    const float* l0_ready;
    void* obs_bf16_ahead;
    int64_t ld_obs_bf16_ahead;
    /* header v7, transition sink with DEFERRED values (t_rewards set, t_values NULL): nothing inside a rollout consumes V(s_t) except the
     * time-out bootstrap r += gamma * V * time_outs (ppo.py:107-108) and the GAE that follows the rollout, and the weights do not change
     * while it is collected -- so the critic may run ONCE over all stored rows afterwards (hgym_critic_values) instead of once per
     * step.  The finaliser then stores the RAW reward in t_rewards and, here, the flags the bootstrap would have used (the stale-by-design
     * extras["time_outs"] of this step, (N,) uint8); hgym_gae_bootstrap applies the same fp32 expression when it loads r_t. */
    uint8_t* t_time_outs;
} HgymEnvOut;
#define HGYM_LOG_STATS 256
#define HGYM_LOG_TERMS 0         /* 22 slots */
#define HGYM_LOG_STEPS 22
#define HGYM_LOG_CLEAR 23        /* the caller clears [0, HGYM_LOG_CLEAR) after reading */
#define HGYM_LOG_RING_HEAD 24
#define HGYM_LOG_RING_FILL 25
#define HGYM_LOG_RING 100        /* entries of each of the two rings */
#define HGYM_LOG_RETURNS 32
#define HGYM_LOG_LENGTHS 132

/* Optional externally supplied random draws (parity mode), row-major (N,k) tables indexed by env id.
 * A NULL member means "draw it from the internal Philox4x32-10 stream keyed by (seed, step, env, slot)". */
typedef struct HgymEnvNoise {
    const float* u_delay;      /* (N,)    U[0,1)  humanoid_env.py:194 */
    const float* z_act;        /* (N,12)  N(0,1)  humanoid_env.py:196 */
    const float* u_cmd;        /* (N,6)   U[0,1)  [0:3] callback resample, [3:6] reset resample (legged_robot.py:328-331) */
    const float* u_dof;        /* (N,12)  U[0,1)  legged_robot.py:367 */
    const float* u_push;       /* (N,5)   U[0,1)  humanoid_env.py:88-93 */
    const float* z_obs;        /* (N,47)  N(0,1)  humanoid_env.py:251 */
    const float* u_xy;         /* (N,2)   U[0,1)  legged_robot.py:385 (custom origins) */
    const int64_t* r_level;    /* (N,)    integers in [0, terrain_rows)  legged_robot.py:418 (terrain curriculum) */
} HgymEnvNoise;

/* XBotLFreeEnv.__init__ tail (humanoid_env.py:78-81): state defaults, reset_idx(all), compute_observations. */
int32_t hgym_env_prime(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st,
                       const HgymEnvOut* out, const HgymEnvNoise* noise, void* stream);

/* LeggedRobot.reset's reset_idx(all) (legged_robot.py:112-114): the reset branch for every env, history
 * cleared, no observation pushed (the caller follows with a zero-action step, :115-116). */
int32_t hgym_env_reset_all(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st,
                           const HgymEnvOut* out, const HgymEnvNoise* noise, void* stream);

/* LeggedRobot.reset_idx(env_ids) (legged_robot.py:163-215 + humanoid_env.py:264-269) for the envs listed in env_ids: n_ids int64
 * DEVICE indices; negative ids wrap as torch indexing does, ids outside [-N, N) are skipped (never dereferenced) and counted in
 * *rejected (a device int64, overwritten); a repeated id resets its env once and counts once in the episode means (the reference's
 * torch.mean counts repeats).  mask_scratch: N device bytes of caller scratch.  Three launches on `stream` (four with the command
 * curriculum), no host synchronisation, capturable.  For the listed envs, in the reference's order: terrain curriculum on the pre-reset root and commands; the command
 * curriculum when common_step_counter % max_episode_length == 0, judged on the listed envs; dofs, root (custom origins), command
 * resample; actions / last_actions / last_last_actions / last_dof_vel / feet_air_time / episode_length zeroed; reset byte = 1;
 * episode sums (built-in and user-defined terms) accumulated, then zeroed; projected_gravity and base_euler of the new pose; both
 * history rings zeroed for those rows.  Every other env keeps every state field, sim tensor row, ring row and reset byte bit for
 * bit.  No observation is written (the reference's reset_idx computes none).  Finaliser: extras_episode / extras_custom = mean
 * over the reset envs / episode_length_s and extras_time_outs = time_out, unchanged when no env was reset; counters[HGYM_CNT_STEP] and [HGYM_CNT_RING] do
 * not move, counters[HGYM_CNT_RESETS] is cleared, counters[HGYM_CNT_RESET_CALL] advances; the transition and logging sinks of `out` are not touched.
 * Draws: the internal Philox stream keyed by (seed, counters[HGYM_CNT_RESET_CALL], env, slot) with bit 30 of the high step word set -- words no step
 * draw uses, so two host resets, or a host reset and the next step's reset of the same env, draw different numbers.  `noise`
 * tables (u_dof, u_cmd[:, 3:6], u_xy, r_level; indexed by env id) override the draws as for the step.
 * Precondition: no step finaliser is pending (HgymEnvOut.defer_finalize) and no fused rollout is between hgym_rollout_begin and
 * hgym_rollout_end (their carried rows assume nobody writes the state in between). */
int32_t hgym_env_reset_idx(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, const HgymEnvOut* out,
                           const HgymEnvNoise* noise, const int64_t* env_ids, int32_t n_ids, uint8_t* mask_scratch, int64_t* rejected,
                           void* stream);

/* XBotLFreeEnv.step head + LeggedRobot.step clip (humanoid_env.py:189-197, legged_robot.py:90-91):
 * st->actions <- clip(blend(clip(actions_in), st->actions) * (1 + noise)).  actions_in (N,12) row-major; read-only
 * unless cfg->use_ref_actions, in which case the reference pose is added to it in place first (as the reference does to
 * the caller's tensor). */
int32_t hgym_pre_physics(const HgymEnvConfig* cfg, const HgymEnvState* st, float* actions_in,
                         const HgymEnvNoise* noise, void* stream);

/* LeggedRobot._compute_torques (legged_robot.py:340-356) on the current dof state -> st->torques. */
int32_t hgym_pd_torques(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, void* stream);

/* Stands where gym.simulate x decimation is (legged_robot.py:94-101,124-126): the synthetic physics of
 * SURVEY.md §8d (benchmark backend).  Runs `decimation` PD + semi-implicit Euler substeps and draws the
 * root / contact / rigid-body tensors from Philox. */
int32_t hgym_synth_physics(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, void* stream);

/* LeggedRobot.post_physics_step + obs clip (legged_robot.py:119-151,105-108) with XBotLFreeEnv's
 * callbacks, 22 reward terms, mask-driven reset_idx and observation stacking. */
int32_t hgym_post_physics(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st,
                          const HgymEnvOut* out, const HgymEnvNoise* noise, void* stream);

/* Fast path: pre_physics + synth_physics + post_physics in ONE launch, then the step finaliser. */
int32_t hgym_env_step_synth(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st,
                            const HgymEnvOut* out, float* actions_in, void* stream);

/* One env step in TWO launches, for tasks with user-defined reward terms (HgymEnvConfig.num_custom_rewards > 0):
 *   hgym_env_step_begin  action processing (+ synthetic physics when actions_in != NULL; NULL: an external simulator has written the
 *                        sim tensors, as for hgym_post_physics), episode length + 1, derived state, command resampling, pushes,
 *                        termination flags -> out->reset / out->time_out -- legged_robot.py:128-137,156-161: the state
 *                        compute_reward (:142) starts from;
 *   [the caller evaluates its `_reward_<name>` terms on that state and writes term * scale * dt into st->custom_rew]
 *   hgym_env_step_end    compute_reward with the caller's terms merged in at their alphabetical positions, reset_idx,
 *                        observations, tail, finaliser (:142-151).
 * With num_custom_rewards == 0 the pair computes exactly what hgym_env_step_synth / hgym_post_physics do in one launch. */
int32_t hgym_env_step_begin(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, const HgymEnvOut* out,
                            const HgymEnvNoise* noise, float* actions_in, void* stream);
int32_t hgym_env_step_end(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, const HgymEnvOut* out,
                          const HgymEnvNoise* noise, void* stream);

/* LeggedRobot._get_heights (legged_robot.py:761-795) for the poses the last env step left in st->height_pose ->
 * st->measured_heights.  The env-step entry points call it themselves when cfg->num_height_points > 0. */
int32_t hgym_measure_heights(const HgymEnvConfig* cfg, const HgymEnvState* st, void* stream);

/* The step finaliser of the last env step on its own (flushes HgymEnvOut.defer_finalize; a no-op to call twice it is NOT:
 * the counters advance each time). */
int32_t hgym_env_finalize(const HgymEnvConfig* cfg, const HgymEnvState* st, const HgymEnvOut* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rollout storage side (algo/ppo/rollout_storage.py, algo/ppo/ppo.py:103-117)
 * ---------------------------------------------------------------------------------------------- */

/* PPO.process_env_step + RolloutStorage.add_transitions for the scalar columns (ppo.py:103-113,
 * rollout_storage.py:87-100): rewards_slot = rew + gamma*values*time_outs ; dones_slot = dones. */
int32_t hgym_store_step(int32_t n, const float* rew, const float* values, const uint8_t* time_outs,
                        const uint8_t* dones, float gamma, float* rewards_slot, uint8_t* dones_slot, void* stream);

/* The minibatch permutation of RolloutStorage.mini_batch_generator (rollout_storage.py:149, torch.randperm(T*N)): out[i], i in
 * [0, n), is a bijection of [0, n) keyed by (seed, draw) -- a 6-round Feistel network, cycle-walked; one launch, no scratch
 * (torch.randperm on the device: a sort, 125 us per iteration at the XBot-L batch). */
int32_t hgym_randperm(int64_t n, uint64_t seed, uint64_t draw, int64_t* out, void* stream);
/* header v9: the same permutation with the draw number read from DEVICE memory (*draw, one int64 the caller advances with a device
 * operation): the launch's arguments do not change from one learning iteration to the next, so an update captured into a HIP graph
 * (OnPolicyRunner: the whole iteration is two graph replays) draws a new permutation at every replay. */
int32_t hgym_randperm_dev(int64_t n, uint64_t seed, const int64_t* draw, int64_t* out, void* stream);

/* RolloutStorage.compute_returns (rollout_storage.py:122-136): GAE(lambda) as a wavefront suffix scan.
 * rewards/values/returns/advantages are (T,N) time-major fp32, dones (T,N) uint8, last_values (N,).
 * stats: HGYM_GAE_STATS_DOUBLES(n) doubles on the device, ZERO-FILLED ONCE by the caller: [0] sum adv, [1] sum adv^2, [2] count are
 * WRITTEN by the call; [3] is the arrival counter of the call's workgroups (left zero again), [4 ..) their partial sums, which the
 * last workgroup to arrive adds up in workgroup order -- the statistics have the same bits in every run and on every rank (header v8;
 * until v7 three doubles accumulated with fp64 atomics in arrival order).  One call at a time per stats buffer. */
#define HGYM_GAE_STATS_DOUBLES(n) (4 + 2 * (((n) + 15) / 16))
int32_t hgym_gae(int32_t T, int32_t n, const float* rewards, const float* values, const uint8_t* dones,
                 const float* last_values, float gamma, float lam, float* returns, float* advantages,
                 double* stats, void* stream);

/* advantages = (adv - mean) / (std_unbiased + 1e-8) from stats (possibly all-reduced by the caller). */
int32_t hgym_adv_normalize(int64_t count, float* advantages, const double* stats, void* stream);

/* Advantages standardised PER MINIBATCH (rsl_rl's normalize_advantage_per_mini_batch; PPO.advantage_normalization = "minibatch"), one
 * segmented pass for all minibatches of an update.  Segment s is idx[s * seg_len, (s + 1) * seg_len), s < segments:
 *     out[idx[j]] = (adv[idx[j]] - mean_s) / (std_s + 1e-8f),   mean_s / std_s (unbiased) over the seg_len gathered values of segment s
 * in hgym_adv_normalize's arithmetic: fp64 sum and sum of squares of the fp32 values, mean = (float)(s1 / n), var = (s2 - s1 s1 / n) /
 * (n - 1) clamped at 0, denom = (float)sqrt(var) + 1e-8f, the result (adv - mean) / denom in fp32.  A constant segment gives exactly 0.
 * The sums are formed per chunk of 1024 consecutive entries of a segment by a fixed tree and added in chunk order: the same bits in every
 * run, no fp64 atomics.  Two launches, no allocation, no host synchronisation, the same arguments in every iteration (capturable).
 * idx: a DEVICE array of segments * seg_len DISTINCT row numbers in [0, rows) -- the caller's guarantee (a slice of the update's
 * permutation); the library cannot validate it without a host synchronisation, and an entry outside [0, rows) reads and writes nothing.
 * adv, out: columns of `rows` floats each, not overlapping; rows of out that no entry names are not touched.
 * scratch: HGYM_ADV_MB_SCRATCH_DOUBLES(segments, seg_len) doubles on the device, ZERO-FILLED ONCE by the caller (per segment: sum, sum of
 * squares, the arrival counter of the segment's chunks, left zero again; behind them the chunks' partial sums).  One call at a time per
 * scratch buffer.
 * Nothing launched and HGYM_E_SHAPE: segments < 1, seg_len < 2 (one value has no unbiased deviation; rsl_rl would produce NaN), rows <
 * segments * seg_len.  HGYM_E_UNSUPPORTED: segments * seg_len > 2^40.  HGYM_E_BADARG: a null pointer, adv and out overlapping within rows. */
#define HGYM_ADV_MB_SCRATCH_DOUBLES(segments, seg_len) ((int64_t)(segments) * (3 + 2 * (((int64_t)(seg_len) + 1023) / 1024)))
int32_t hgym_adv_normalize_minibatches(int32_t segments, int64_t seg_len, const int64_t* idx, const float* adv, float* out, int64_t rows,
                                       double* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Value targets standardised by running statistics (PPO.value_normalization; rl_games' normalize_value, the return half of SB3's
 * VecNormalize; header v9, no layout changes).  The critic lives in normalised units; around GAE three scalar
 * columns change units.
 *   block     HGYM_VALUE_NORM_BLOCK_DOUBLES doubles of the caller on the device, 8-byte aligned: [0] count, [1] mean, [2] var (population
 *             variance).  The caller writes the initial state 0, 0, 1; hgym_value_norm_merge is the only writer afterwards.
 *   floats    mean_f = (float)mean, scale_f = (float)sqrt(var) + eps, formed by every call from the block; eps >= 0 and finite.
 *   denormalise   V = v * scale_f + mean_f        fp32, two roundings (no fma)
 *   normalise     y = (x - mean_f) / scale_f      fp32, two roundings, the division correctly rounded
 *   merge     of a batch of n fp32 values with mean_b and population variance var_b, in fp64, rsl_rl's EmpiricalNormalization merge as
 *             hgym_net_norm_merge does it:
 *                 count' = count + n;  rate = n / count';  d = mean_b - mean;  mean' = mean + rate * d;
 *                 var' = var + rate * (var_b - var + d * (mean_b - mean')), clamped at 0
 *             From count = 0 the formula's value IS the batch's statistics: the call then stores mean' = mean_b, var' = var_b themselves (in
 *             floating point 1 + (var_b - 1) would round).
 *   batch statistics   chunk-wise (n, mean, M2) combined by Chan's rule; no sum of raw squares is formed, so the variance survives
 *             |mean| >> std.  Per chunk of HGYM_VALUE_NORM_CHUNK consecutive values, two passes in fp64: mean_c = (sum x) / n_c, then
 *             M2_c = sum (x - mean_c)^2, each sum by a fixed tree.  The chunks' (n_c, mean_c, M2_c) are combined pairwise in a fixed order,
 *                 n = n_a + n_b;  d = mean_b - mean_a;  mean = mean_a + d * (n_b / n);  M2 = M2_a + M2_b + d * d * (n_a * n_b / n),
 *             by the last workgroup to arrive (a counter in the scratch, left zero again): no fp64 atomics, the same inputs give the same
 *             bits in every run.  var_b = M2 / n.
 *   scratch   HGYM_VALUE_NORM_SCRATCH_DOUBLES(n) doubles on the device, 8-byte aligned, ZERO-FILLED ONCE by the caller:
 *             [HGYM_VALUE_NORM_BATCH + 0 .. 2] the batch's raw n, mean_b, var_b as the last call left them (what a multi-rank exchange would
 *             carry between "batch statistics" and "merge"), [HGYM_VALUE_NORM_TICKET] the arrival counter, [HGYM_VALUE_NORM_PARTIALS ..)
 *             mean_c, M2_c per chunk.  One call at a time per scratch buffer.
 * Every call: ONE launch on `stream`, ceil(n / HGYM_VALUE_NORM_CHUNK) workgroups up to HGYM_VALUE_NORM_MAX_BLOCKS (which then walk the
 * chunks with that stride), no allocation, no host synchronisation, the same arguments in every iteration (capturable).  16-byte loads and
 * stores where the columns are 16-byte aligned, 4-byte ones otherwise.
 *   hgym_value_denormalize   dst[i] = src[i] * scale_f + mean_f, i < n.  dst == src is allowed; any other overlap is HGYM_E_BADARG.
 *   hgym_value_norm_merge    the statistics of returns[0 .. n) -> scratch, merged into block.
 *   hgym_value_normalize     x[i] = (x[i] - mean_f) / scale_f in place, i < n.
 * Nothing launched and HGYM_E_SHAPE: n < 1.  HGYM_E_UNSUPPORTED: n > 2^40.  HGYM_E_BADARG: a null pointer, block or scratch not 8-byte
 * aligned, a column not 4-byte aligned, eps negative or not finite. */
#define HGYM_VALUE_NORM_BLOCK_DOUBLES 3
#define HGYM_VALUE_NORM_CHUNK 1024
#define HGYM_VALUE_NORM_MAX_BLOCKS 1024
#define HGYM_VALUE_NORM_BATCH 0
#define HGYM_VALUE_NORM_TICKET 3
#define HGYM_VALUE_NORM_PARTIALS 4
#define HGYM_VALUE_NORM_SCRATCH_DOUBLES(n) (HGYM_VALUE_NORM_PARTIALS + 2 * (((int64_t)(n) + HGYM_VALUE_NORM_CHUNK - 1) / HGYM_VALUE_NORM_CHUNK))
int32_t hgym_value_denormalize(int64_t n, const float* src, float* dst, const double* block, float eps, void* stream);
int32_t hgym_value_norm_merge(int64_t n, const float* returns, double* block, double* scratch, void* stream);
int32_t hgym_value_normalize(int64_t n, float* x, const double* block, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Random Network Distillation's reward pass (rsl_rl's rnd_cfg; PPO.rnd; header v9, no layout changes).
 * Behind a rollout the caller runs a frozen target net and a trained predictor over the NEXT state of every stored transition (storage
 * slots 1 .. T); this call turns the two embeddings into a normalised, scheduled exploration reward and adds it to the stored rewards,
 * ahead of GAE.
 *   pred, target   (T * n, K) fp32, row-major, contiguous; row t * n + i is transition t of env i.  1 <= K <= HGYM_RND_MAX_OUTPUTS.
 *   rewards        (T, n) fp32, updated in place.        err, intrinsic   (T, n) fp32, written.
 *   block          HGYM_RND_BLOCK_DOUBLES(n) doubles of the caller, written once by hgym_rnd_block_init; the state carried from call to call.
 * Arithmetic, every operation rounded once:
 *   raw error      e[t][i] = sqrtf(sum_j (target_j - pred_j)^2): differences, squares and the sum in fp32, the sum starting from 0 with j
 *                  ascending, the square root correctly rounded (torch.linalg.norm(target - predictor, dim=1)).
 *   discounted average, per env, fp64, carried ACROSS calls in block[HGYM_RND_HEADER + i]:
 *                  G_i = gamma * G_i + (double)e[t][i]   for t = 0 .. T - 1; no reset on episode ends (rsl_rl's DiscountedAverage has none).
 *   running statistics of G, (mean, var, count) = (0, 1, 0) after hgym_rnd_block_init: the call's T * n values of G are ONE batch of
 *                  nb = T * n values with mu_b = sum G / nb and var_b = sum G^2 / nb - mu_b^2 clamped at 0, merged FIRST, by the formula stated
 *                  for hgym_net_norm_merge:
 *                      count += nb;  rate = nb / count;  d = mu_b - mean;  mean += rate * d;  var += rate * (var_b - var + d * (mu_b - mean_new))
 *                  The two sums are fp64 partial sums per HGYM_RND_ENVS_PER_PARTIAL envs (per env t ascending; the envs of a partial by a
 *                  fixed tree), added in a fixed order: no fp64 atomics, the same inputs give the same bits in every run.  std = sqrt(var).
 *   weight         row t uses the step count c = counter + t + 1, counter = block[HGYM_RND_COUNTER] (an integer in a double slot; the call
 *                  leaves counter += T), in fp64:
 *                      HGYM_RND_CONSTANT  w = weight
 *                      HGYM_RND_STEP      w = weight while c < final_step, then final_value
 *                      HGYM_RND_LINEAR    w = weight for c <= initial_step, final_value for c >= final_step, between them
 *                                         weight + (final_value - weight) * (double)(c - initial_step) / (double)(final_step - initial_step),
 *                                         evaluated left to right
 *   applying it    scale_t = (float)(normalize && std > 0 ? w / std : w);  intrinsic[t][i] = e[t][i] * scale_t, one fp32 product;
 *                  rewards[t][i] += intrinsic[t][i], one fp32 addition.  normalize = 0: the statistics are kept, scale_t = (float)w.
 *   logging        written, not accumulated: block[HGYM_RND_SUM_INTRINSIC] = sum of (double)intrinsic, block[HGYM_RND_SUM_REWARDS] = sum of the
 *                  (double) incoming rewards (both over all T * n entries, ordered partial sums), block[HGYM_RND_WEIGHT_LAST] = w of row
 *                  T - 1, block[HGYM_RND_STD] = std, block[HGYM_RND_ROWS] = T * n.
 * The block: [HGYM_RND_MEAN], [HGYM_RND_VAR], [HGYM_RND_COUNT], [HGYM_RND_COUNTER], the five logging slots, two arrival counters (integers in
 * the first word of their slots, zero between calls), HGYM_RND_HEADER doubles in all; then G [n]; then scratch of the launches.
 * Rows-per-workgroup of the launches (informational, for tests that sit on the edges): HGYM_RND_ROWS_PER_WG rows of the embeddings,
 * HGYM_RND_ENVS_PER_PARTIAL envs of the average, 256 envs of one row when applying.
 * hgym_rnd_block_init writes every double of the block (mean 0, var 1, everything else 0).  Both calls enqueue on `stream`; nothing
 * synchronises, nothing allocates; with fixed arguments hgym_rnd_rewards is capturable (three launches).  One call at a time per block.
 * HGYM_E_BADARG and nothing launched: a null pointer; T, n or K < 1; K > HGYM_RND_MAX_OUTPUTS; gamma outside [0, 1); a schedule other than the
 * three; weight (and, where the schedule reads it, final_value) negative or not finite; HGYM_RND_LINEAR with final_step <= initial_step;
 * normalize outside {0, 1}.
 * ---------------------------------------------------------------------------------------------- */
#define HGYM_RND_MAX_OUTPUTS 64
#define HGYM_RND_CONSTANT 0
#define HGYM_RND_STEP 1
#define HGYM_RND_LINEAR 2
#define HGYM_RND_HEADER 16
#define HGYM_RND_MEAN 0
#define HGYM_RND_VAR 1
#define HGYM_RND_COUNT 2
#define HGYM_RND_COUNTER 3
#define HGYM_RND_SUM_INTRINSIC 4
#define HGYM_RND_SUM_REWARDS 5
#define HGYM_RND_WEIGHT_LAST 6
#define HGYM_RND_STD 7
#define HGYM_RND_ROWS 8
#define HGYM_RND_TICKET_SCAN 9
#define HGYM_RND_TICKET_APPLY 10
#define HGYM_RND_ROWS_PER_WG 64
#define HGYM_RND_ENVS_PER_PARTIAL 64
#define HGYM_RND_APPLY_WGS 1024
#define HGYM_RND_BLOCK_DOUBLES(n) ((size_t)HGYM_RND_HEADER + (size_t)(n) + 2 * (((size_t)(n) + HGYM_RND_ENVS_PER_PARTIAL - 1) / HGYM_RND_ENVS_PER_PARTIAL) + 2 * (size_t)HGYM_RND_APPLY_WGS)
typedef struct {
    double gamma;          /* discount of the per-env average G, in [0, 1) */
    double weight;         /* the (initial) weight, finite and >= 0 */
    double final_value;    /* HGYM_RND_STEP / HGYM_RND_LINEAR: the weight from final_step on */
    int64_t initial_step;  /* HGYM_RND_LINEAR */
    int64_t final_step;    /* HGYM_RND_STEP / HGYM_RND_LINEAR */
    int32_t schedule;      /* HGYM_RND_CONSTANT / HGYM_RND_STEP / HGYM_RND_LINEAR */
    int32_t normalize;     /* 1: divide by the running deviation of G (rsl_rl's reward_normalization); 0: the statistics are kept but not used */
} HgymRndConfig;
int32_t hgym_rnd_block_init(int32_t n, double* block, void* stream);
int32_t hgym_rnd_rewards(int32_t T, int32_t n, int32_t K, const float* pred, const float* target, float* rewards, float* err, float* intrinsic,
                         const HgymRndConfig* cfg, double* block, void* stream);

/* hgym_gae for a rollout collected with deferred values (HgymEnvOut.t_time_outs): rewards (T, n) holds the RAW rewards and is
 * overwritten with r_t + gamma * (V_t * time_outs_t) -- PPO.process_env_step's bootstrap (ppo.py:107-108), the three fp32 roundings of
 * hgym_store_step -- before the scan uses it, so that afterwards every storage column is what the per-step path leaves. */
int32_t hgym_gae_bootstrap(int32_t T, int32_t n, float* rewards, const float* values, const uint8_t* dones, const uint8_t* time_outs,
                           const float* last_values, float gamma, float lam, float* returns, float* advantages, double* stats, void* stream);

/* Left-right symmetry augmentation (header v9, no layout change; PPO.symmetry): the mirrored copy of M stored
 * rows.  For every row m and c < width, dst[m * ld_dst + c] is the BIT PATTERN of src[m * ld_src + src_col[c]] with the sign bit inverted
 * where sign[c] < 0 -- a flip, not a multiply, so the call is exact for every input (NaN payloads, denormals, +-0, +-inf) and the bf16
 * mirror of a shadow row equals bf16(mirror(fp32 row)) bit for bit.  Columns [width, zero_to) of every dst row are written as +0 (the
 * pad columns of a shadow; zero_to = width: none); columns [zero_to, ld_dst) are not touched.  dtype: HGYM_F32 (4-byte elements) or
 * HGYM_BF16 (2-byte); ld_src / ld_dst in elements.  Rows need only be aligned to their element (705 floats are 2820 bytes); 16-byte
 * accesses are used wherever the addresses allow.  src_col (width int32) and sign (width floats) are DEVICE arrays of the caller, read
 * by the launch: the library cannot validate their contents (the Python layer does, humanoid/utils/symmetry.py: MirrorSpec); an entry
 * outside [0, width) reads the row's last column.  The table need not be an involution.
 * HGYM_E_BADARG, and nothing launched: a null pointer, M < 0, width < 1, ld_src or ld_dst < width, zero_to outside [width, ld_dst], a
 * pointer not aligned to its element, an unknown dtype, or src and dst ranges that overlap.  HGYM_E_UNSUPPORTED: zero_to (hence width)
 * > HGYM_MIRROR_MAX_WIDTH -- the kernel stages whole rows and the table in LDS -- or M > 2^40, ld > 2^20.  M = 0: HGYM_OK, no launch. */
#define HGYM_MIRROR_MAX_WIDTH 2048
int32_t hgym_mirror_rows(int64_t M, int32_t width, const int32_t* src_col, const float* sign, const void* src, int64_t ld_src, void* dst,
                         int64_t ld_dst, int32_t zero_to, int32_t dtype /* HGYM_F32 | HGYM_BF16 */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Actor / critic (algo/ppo/actor_critic.py) and PPO update (algo/ppo/ppo.py:119-184)
 * ---------------------------------------------------------------------------------------------- */
enum { HGYM_F32 = 0, HGYM_BF16 = 1 };

/* Activation between the Linear layers of the actor, the critic and the auxiliary head (the reference's
 * ActorCritic(activation=...), actor_critic.py:41; one module for every MLP).  HgymNetConfig.act_alpha / act_scale:
 *   HGYM_ACT_ELU         scale * (z > 0 ? z : alpha * (exp(z) - 1));  alpha 0 -> 1, scale 0 -> 1 (nn.ELU(alpha))
 *   HGYM_ACT_SELU        the same form; alpha 0 -> 1.6732632423543772, scale 0 -> 1.0507009873554805 (nn.SELU)
 *   HGYM_ACT_LEAKY_RELU  z > 0 ? z : alpha * z;  alpha = the negative slope >= 0 (0: nn.ReLU), act_scale 0
 *   HGYM_ACT_TANH, HGYM_ACT_SIGMOID   act_alpha = act_scale = 0
 * The backward takes the derivative from the stored output y = f(z) (ELU: y > 0 ? scale : y + scale * alpha; LeakyReLU: y > 0 ?
 * 1 : alpha; Tanh: 1 - y^2; Sigmoid: y (1 - y)), so no kind needs more workspace than another.  Anything else (an unknown kind,
 * alpha or scale < 0, a parameter a kind does not use set) is refused by hgym_net_param_count / hgym_net_workspace_bytes and
 * every call taking the configuration.
 * Supported: every kind at HGYM_F32 and HGYM_BF16 on the layer-by-layer GEMM path.  The fused bf16 kernels take ELU(1), and every
 * other kind when HgymNetConfig.fused_activation = 1 (hgym_rollout_step: in its values = NULL form); without it a
 * bf16 configuration with another activation runs the GEMM path, as a net too wide for the fused tiles' LDS does. */
enum { HGYM_ACT_ELU = 0, HGYM_ACT_SELU = 1, HGYM_ACT_LEAKY_RELU = 2, HGYM_ACT_TANH = 3, HGYM_ACT_SIGMOID = 4 };

/* What slots [0, num_actions) of the flat parameter vector hold (HgymNetConfig.std_param):
 *   HGYM_STD_SCALAR  the standard deviations sigma themselves (the reference's `std`, actor_critic.py:80; nothing keeps them positive)
 *   HGYM_STD_LOG     log sigma; sigma = exp(log sigma) is positive wherever the optimiser moves the parameter, and an Adam step is a
 *                    relative change of sigma (noise_std_type = "log" of current rsl_rl)
 * In HGYM_STD_LOG the library keeps sigma[j] = expf(params[j]), j < num_actions, in a block of 16 floats of the workspace
 * (hgym_net_sigma_offset) and every kernel reads sigma from there -- the same kernels, the same arithmetic, the same bits as
 * HGYM_STD_SCALAR with those values as parameters.  The block is rewritten where the parameter changes and nowhere else: by
 * hgym_ppo_apply (inside the Adam launch, so a captured update keeps it current) and by hgym_net_sync_shadow (call it after writing
 * params, as for the operand copies; until the first of the two the block is the zero fill).  The gradient of slots [0, num_actions)
 * is that of the parameter: d/d(log sigma) = fp32(d/d sigma) * sigma, one fp32 product applied where hgym_ppo_grad / hgym_ppo_grad_part
 * (part 0, ahead of a rank exchange) write it, so the squared norm in opt_state[HGYM_OPT_GRAD_SQNORM] and the clip are the parameter's too. */
enum { HGYM_STD_SCALAR = 0, HGYM_STD_LOG = 1 };

typedef struct HgymNetConfig {
    int32_t num_obs, num_priv, num_actions;
    int32_t actor_layers, critic_layers;                 /* number of Linear layers (4, 4) */
    int32_t actor_dims[HGYM_MAX_LAYERS + 1];             /* 705,512,256,128,12 */
    int32_t critic_dims[HGYM_MAX_LAYERS + 1];            /* 219,768,256,128,1  */
    int32_t precision;                                   /* HGYM_F32 (parity) or HGYM_BF16 (MFMA fast path) */
    int32_t max_batch;                                   /* largest M any call will use */
    /* Optional auxiliary head trained jointly with PPO (BASELINE configs[4], SURVEY.md 8f item 4: the denoising world-model
     * head -- NO reference code exists for it; design: DESIGN.md section 9).  An MLP obs -> aux_dims[1..] (`activation` between) that
     * regresses columns [aux_target_offset, aux_target_offset + aux_dims[aux_layers]) of the privileged observation row
     * with a mean-squared error weighted by HgymPPOConfig.aux_coef.  aux_layers = 0: absent.  Its parameters follow the
     * critic's in the flat vector ("denoiser.{0,2,..}.{weight,bias}"); hgym_mlp_forward(which = 2) evaluates it. */
    int32_t aux_layers;
    int32_t aux_dims[HGYM_MAX_LAYERS + 1];               /* aux_dims[0] = num_obs */
    int32_t aux_target_offset;
    int32_t activation;                                  /* HGYM_ACT_* (0: ELU, the reference default) */
    float act_alpha, act_scale;                          /* its parameters, see HGYM_ACT_* (0, 0: the kind's defaults) */
    int32_t std_param;              /* HGYM_STD_* above: HGYM_STD_SCALAR (0, the default) -- params[0 .. num_actions) are sigma; HGYM_STD_LOG (1) --
                                       they are log sigma.  The outputs named `sigma` and `std` of every call are sigma in both modes, never
                                       its logarithm.  Any other value: HGYM_E_BADARG from every call taking the configuration.  Added
                                       later within header v9, AHEAD of fused_activation, which stays the last field of the struct (its
                                       mirrors and their tests locate it as the struct's last four bytes): a zero-filled field is
                                       HGYM_STD_SCALAR, and a caller built against an earlier v9 header is rebuilt against this one, as
                                       for every field the struct has gained (hgym_sizeof("HgymNetConfig") tells a stale mirror). */
    int32_t fused_activation;       /* which activations take the fused bf16 kernels (forward tiles, the update's fused tiles, the bf16
                                         observation shadow), in a bf16 configuration those kernels accept:
                                         0: ELU(1) only; every other activation runs the layer-by-layer GEMM path  (the default)
                                         1: any resolved activation, through the kernels' generic instantiation: hardware exp2 / rcp forms
                                            where the GEMM path calls libm, so the two paths round differently (both within the bf16 bars).
                                            With ELU(1) it changes nothing: same kernels, same bits.  hgym_rollout_eval_step and
                                            hgym_rollout_step with values = NULL serve such a net; hgym_rollout_step WITH the critic's
                                            tiles (values != NULL) is built for ELU(1) only and returns HGYM_E_UNSUPPORTED.
                                       Ignored wherever the fused kernels are refused anyway (HGYM_F32, widths they do not take, an
                                       auxiliary head outside their shapes).  Any other value: HGYM_E_BADARG from every call taking the
                                       configuration.  Appended later within header v9, so a zero-filled tail is ELU(1) only. */
} HgymNetConfig;

typedef struct HgymPPOConfig {
    float clip_param, value_loss_coef, entropy_coef, max_grad_norm, desired_kl;
    float beta1, beta2, adam_eps;
    double lr_min, lr_max;          /* 1e-5, 1e-2 (ppo.py:142-145) */
    int32_t adaptive_lr;            /* schedule == 'adaptive' */
    int32_t world_size;             /* >1: between hgym_ppo_grad and hgym_ppo_apply the caller all-reduces (SUM) the P+1 floats of
                                       net->grads across ranks; apply forms the means (gradient and KL) itself */
    float aux_coef;                 /* weight of the auxiliary head's MSE in the total loss (0 with aux_layers = 0) */
    int32_t grad_norm_ready;        /* 1: net->grads is exactly what the preceding hgym_ppo_grad left (one rank, nothing touched it),
                                       so its squared norm is already in opt_state[9] (GRAD_SQNORM) and apply skips its own pass over the
                                       gradient; 0 (or world_size > 1): apply computes the norm itself.  The flag is a PROMISE that every
                                       hgym_ppo_grad is followed by exactly one hgym_ppo_apply with the same configuration: on the fused
                                       bf16 path hgym_ppo_grad then also takes the adaptive-KL learning-rate decision and advances Adam's
                                       step count (the work of apply's prologue, done beside the weight-gradient launch).  A marker in
                                       opt_state[13] (PROLOGUE_STEP) keeps the two honest: a second hgym_ppo_grad before the apply does not advance the step
                                       again, and an apply under another configuration does not repeat a prologue already taken.  (Not
                                       covered: a gradient call WITHOUT the flag followed by an apply WITH it -- no prologue runs.) */
    int32_t value_loss_unclipped;   /* the value loss (the reference's use_clipped_value_loss, ppo.py:158-166), in every path:
                                         0: max((V - R)^2, (V_old + clamp(V - V_old, -clip, clip) - R)^2).mean()  (the reference default)
                                         1: (R - V)^2.mean()  (use_clipped_value_loss = False)
                                       opt_state[4] (VALUE_SUM) sums the form in use.  Any other value: HGYM_E_BADARG from every call taking the
                                       configuration.  Appended later within header v9, so a zero-filled tail is the clipped form. */
    float mirror_coef;              /* weight of the mirror loss (rsl_rl's symmetry_cfg: use_mirror_loss / mirror_loss_coeff).
                                       For a minibatch of B rows with A actions, row b = storage row idx[b] with partner row pair_idx[b] (the
                                       mirrored observation of the same transition):
                                           t_b = M_a(mu(obs[pair_idx[b]]))      current parameters, NO gradient through t_b
                                           L_m = mirror_coef / (B A) * sum_b sum_j (mu(obs[idx[b]])_j - t_bj)^2
                                       with M_a(y)_j = mirror_act_sign[j] * y[mirror_act_src[j]].  L_m is added to the PPO loss: it changes d mu
                                       (hence the actor's gradients) and nothing else -- d std, the critic, the auxiliary head, the KL of the
                                       learning-rate rule and the loss sums of opt_state are what they are without it.  0: off -- the five
                                       HgymBatch members below are ignored, the launches and every output bit are those of a library without the
                                       feature.  > 0: hgym_ppo_grad / hgym_ppo_grad_part (part 0) first run one forward-only actor pass over
                                       obs[pair_idx] (the fp32 rows, on every path) into HgymBatch.mirror_target.  Negative, NaN or infinite:
                                       HGYM_E_BADARG from every call taking the configuration, nothing launched.  Appended later within header
                                       v9, so a zero-filled tail is off. */
} HgymPPOConfig;

/* Sizes (bytes) of the caller-allocated blocks, as functions of the configuration. */
int64_t hgym_net_param_count(const HgymNetConfig* net);          /* 926105 for XBot-L */
int64_t hgym_net_workspace_bytes(const HgymNetConfig* net);
/* byte offset inside the workspace of the derived sigma block (16 floats, the first num_actions in use) with HGYM_STD_LOG; -1 with
 * HGYM_STD_SCALAR (sigma is params[0 .. num_actions) then); -2 for a configuration the library refuses (hgym_last_error says why) */
int64_t hgym_net_sigma_offset(const HgymNetConfig* net);

/* Master parameters are ONE flat fp32 array in state_dict order
 * (std, actor.{0,2,4,6}.{weight,bias}, critic.{0,2,4,6}.{weight,bias}; SURVEY.md §5 checkpoint row; with HgymNetConfig.std_param =
 * HGYM_STD_LOG the first num_actions slots are log_std = log sigma, same place, same count);
 * grads/adam_m/adam_v have the same layout.  opt_state: 16 doubles on the device (HGYM_OPT_* below, one name per slot)
 * [0] learning rate (python-double semantics of ppo.py:142-148)   [1] Adam step count
 * [2] sum of minibatch mean KL  [3] sum of surrogate losses  [4] sum of value losses  [5] sum of mean entropies
 * [6] gradient norm of the last step (before clipping)  [7] minibatches accumulated in [2..5]
 * [8] mean KL of the last minibatch, rounded to fp32 like the reference's kl_mean, which the learning-rate rule compares in fp32
 *     (average it across ranks before hgym_ppo_apply when world_size > 1)
 * [9] internal  [10] sum of the auxiliary head's minibatch MSE losses  [11] Adam step size lr / (1 - beta1^t) and
 * [12] sqrt(1 - beta2^t) of the current step (as floats; written by hgym_ppo_apply)  [13..15] internal (the step whose beta^t lie in [14..15] / the
 * "prologue done, not applied" marker: Adam's betas must not change between a gradient call and the apply that follows it).
 * workspace: hgym_net_workspace_bytes() bytes, 256-byte aligned, ZERO-FILLED once by the caller before first use
 * (padding rows/columns of the operand buffers rely on it). */
#define HGYM_OPT_STATE 16
#define HGYM_OPT_LR 0                /* learning rate */
#define HGYM_OPT_STEP 1              /* Adam step count */
#define HGYM_OPT_KL_SUM 2            /* sum of minibatch mean KL */
#define HGYM_OPT_SURROGATE_SUM 3     /* sum of surrogate losses */
#define HGYM_OPT_VALUE_SUM 4         /* sum of value losses */
#define HGYM_OPT_ENTROPY_SUM 5       /* sum of mean entropies */
#define HGYM_OPT_GRAD_NORM 6         /* gradient norm of the last step (before clipping) */
#define HGYM_OPT_MINIBATCHES 7       /* minibatches accumulated in [2..5] and [10] */
#define HGYM_OPT_KL_LAST 8           /* mean KL of the last minibatch, rounded to fp32 */
#define HGYM_OPT_GRAD_SQNORM 9       /* internal: squared norm of the gradient being formed */
#define HGYM_OPT_AUX_SUM 10          /* sum of the auxiliary head's minibatch MSE losses */
#define HGYM_OPT_STEP_SIZE 11        /* lr / (1 - beta1^t), as a float */
#define HGYM_OPT_SQRT_BC2 12         /* sqrt(1 - beta2^t), as a float */
#define HGYM_OPT_PROLOGUE_STEP 13    /* internal: the step whose beta^t lie in the next two / the "prologue done, not applied" marker */
#define HGYM_OPT_BETA1_POW 14        /* internal: beta1^t */
#define HGYM_OPT_BETA2_POW 15        /* internal: beta2^t */
typedef struct HgymNet {
    float* params;
    float* grads;          /* hgym_net_param_count() + 1 floats: the flat gradient, then ONE slot carrying the minibatch mean KL */
    float* adam_m;
    float* adam_v;
    double* opt_state;     /* [HGYM_OPT_STATE] */
    void* workspace;       /* hgym_net_workspace_bytes() bytes, 256-byte aligned */
    void* norm;            /* observation normalisation (below: hgym_net_norm_*): the caller-owned block of hgym_net_norm_layout()[HGYM_NORM_BYTES]
                              bytes, 256-byte aligned; NULL: off -- every launch, argument and result is what it is without the feature.
                              Appended within header v9 as the LAST member: a zero-filled tail is a net without normalisation. */
} HgymNet;

/* re-derive the compute-precision operand copies (padded W and W^T) from the fp32 master parameters;
 * call after loading a checkpoint.  The Adam kernel keeps them current afterwards. */
int32_t hgym_net_sync_shadow(const HgymNetConfig* cfg, const HgymNet* net, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Empirical observation normalisation (rsl_rl's `empirical_normalization`; header v9, HgymNet.norm appended).
 * Every observation column is standardised by a running mean and standard deviation -- as part of the FIRST LAYER:
 *     W ((x - m) o s) + b  =  (W o s) x + (b - (W o s) m),      s = 1 / (std + eps) per column.
 * The kernels keep reading RAW rows.  With HgymNet.norm set, the operand-precision copies of a first-layer weight hold T(w * s[c]) -- written
 * where every operand copy is written, by hgym_ppo_apply's Adam launch and by hgym_net_sync_shadow -- and the first-layer bias the kernels
 * add is the effective bias b'[r] = b[r] - sum_c Wop[r][c] * m[c] (Wop as rounded to the operand type, so that weight rounding acts on x - m;
 * the sum in fp64 in a fixed order, rounded once to fp32), recomputed by one more launch behind both.  The actor, the critic and the auxiliary
 * head all fold; the head shares the actor's statistics and its regression targets stay raw.  params, grads, adam_m / adam_v stay in the
 * NORMALISED parametrisation (what rsl_rl trains): hgym_ppo_grad leaves the gradient of the operand parametrisation, and
 * hgym_net_norm_unfold_grad turns the first-layer weight gradients into the master's in place -- call it behind every hgym_ppo_grad (part 1
 * of hgym_ppo_grad_part), ahead of a rank exchange and of hgym_ppo_apply.  opt_state[HGYM_OPT_GRAD_SQNORM] as the gradient call left it is then not
 * the final gradient's: HgymPPOConfig.grad_norm_ready must be 0 (hgym_ppo_apply refuses 1 with HGYM_E_BADARG when norm is set).
 *
 * Statistics, fp64 on the device, per column; the actor's over num_obs columns, the critic's over num_priv: mean = 0, var = 1, count = 0 at
 * hgym_net_norm_init.  A batch of n rows with population mean mu_b and variance var_b (= sum x^2 / n - mu_b^2, clamped at 0) merges as
 *     count += n;  rate = n / count;  d = mu_b - mean;  mean += rate * d;  var += rate * (var_b - var + d * (mu_b - mean_new))
 * and the kernels' floats are m = (float)mean, s = (float)(1.0 / (sqrt(var) + (double)eps)): a constant column has var = 0 and the finite scale
 * 1 / eps.  `until` >= 0: once count >= until a merge changes nothing (checked on the device); -1: never stops.
 *
 * The block (HgymNet.norm): hgym_net_norm_layout fills layout[HGYM_NORM_LAYOUT] with its size and the byte offsets of its parts -- callable
 * without a device; HGYM_E_* for a configuration the library refuses or rows wider than 1024 columns.  Index k: 0 = actor / obs, 1 = critic / priv.
 *   [HGYM_NORM_BYTES]          size of the block (no zero-fill needed: hgym_net_norm_init writes every part that is read)
 *   [HGYM_NORM_HEADER]         8 doubles: eps, until, count of the actor's statistics, count of the critic's, 4 unused
 *   [HGYM_NORM_MEAN + k], [HGYM_NORM_VAR + k]          fp64 [K]
 *   [HGYM_NORM_MEAN_F + k], [HGYM_NORM_SCALE_F + k]    fp32 [K]: m and s above
 *   [HGYM_NORM_BIAS + i]       fp32 [first width]: effective bias of net i (0 actor, 1 critic, 2 auxiliary head; -1: no such net)
 *   [HGYM_NORM_SUMS]           fp64 [HGYM_NORM_SUMS_DOUBLES] = [n | sum x [num_obs] | sum x^2 [num_obs] | n | sum x [num_priv] | sum x^2 [num_priv]]:
 *                              what hgym_net_norm_accumulate leaves and hgym_net_norm_merge reads.  Several ranks: all-reduce (SUM) these
 *                              doubles between the two calls; every rank then merges the same batch into the same state.
 *   [HGYM_NORM_PARTIALS + k]   scratch of the accumulate launch; [HGYM_NORM_WGS + k] its workgroups for row kind k, [HGYM_NORM_ROWS_PER_WG] the rows
 *                              of one row block (a workgroup walks blocks b, b + WGS, ...): informational, for tests that sit on the edges
 * hgym_net_norm_init       header, mean = 0, var = 1, count = 0, m = 0, s = 1 / (1 + eps), sums = 0.  Follow with hgym_net_sync_shadow.
 *                          eps >= 0 finite, until >= -1, else HGYM_E_BADARG.
 * hgym_net_norm_accumulate the sums of M rows of obs ((M, num_obs)) and priv ((M, num_priv)), row-major, contiguous, 4-byte aligned (16-byte
 *                          aligned bases take the fast path), any M >= 1: OVERWRITES the sums block.  fp64 partial sums per workgroup added in
 *                          a fixed order, no atomics: the same rows give the same bits.  Two launches.
 * hgym_net_norm_merge      the merge above from the sums block, then the refold: first-layer operand copies and effective biases.
 * hgym_net_norm_unfold_grad  G_W[r][c] = (G'_W[r][c] - g_b[r] * m[c]) * s[c] on the first-layer weight gradients of every net, three fp32
 *                          roundings; bias gradients unchanged.
 * hgym_net_sync_shadow refolds as well when norm is set.  Everything is enqueued on `stream`, nothing synchronises, every call is capturable.
 * ---------------------------------------------------------------------------------------------- */
#define HGYM_NORM_LAYOUT 24
#define HGYM_NORM_BYTES 0
#define HGYM_NORM_HEADER 1
#define HGYM_NORM_MEAN 2
#define HGYM_NORM_VAR 4
#define HGYM_NORM_MEAN_F 6
#define HGYM_NORM_SCALE_F 8
#define HGYM_NORM_BIAS 10
#define HGYM_NORM_SUMS 13
#define HGYM_NORM_SUMS_DOUBLES 14
#define HGYM_NORM_PARTIALS 15
#define HGYM_NORM_WGS 17
#define HGYM_NORM_ROWS_PER_WG 19
int32_t hgym_net_norm_layout(const HgymNetConfig* cfg, int64_t* layout);
int32_t hgym_net_norm_init(const HgymNetConfig* cfg, const HgymNet* net, float eps, int64_t until, void* stream);
int32_t hgym_net_norm_accumulate(const HgymNetConfig* cfg, const HgymNet* net, const float* obs, const float* priv, int64_t M, void* stream);
int32_t hgym_net_norm_merge(const HgymNetConfig* cfg, const HgymNet* net, void* stream);
int32_t hgym_net_norm_unfold_grad(const HgymNetConfig* cfg, const HgymNet* net, void* stream);

/* ActorCritic.act_inference / evaluate (actor_critic.py:122-128): which = 0 actor, 1 critic.
 * x (M, in) row-major fp32 with leading dimension ldx; y (M, out) row-major fp32. */
int32_t hgym_mlp_forward(const HgymNetConfig* cfg, const HgymNet* net, int32_t which, int32_t M,
                         const float* x, int64_t ldx, float* y, void* stream);

/* bf16 shadow of the observation rows (optional; the update's fast path).  The update reads every stored observation row twice per
 * epoch -- the forward gathers it, the first layer's weight-gradient product gathers it again -- and only ever in bf16.  A policy
 * launch has each row in hand as bf16 anyway (it converts the fp32 row for its first layer), so it can leave that copy behind:
 * `shadow->obs` / `shadow->priv` receive, row m, the bf16 of row m of `obs` / `priv` (row-major, leading dimensions ld_obs /
 * ld_priv in elements = hgym_net_shadow_ld(cfg, 0 / 1): the input width padded to 128, pad columns written as zero).  Handed
 * back through HgymBatch.obs_bf16 / priv_bf16, the update gathers 2 bytes per element instead of 4 and writes no operand copy
 * of its own.  NULL: no shadow is written.  Only the fused bf16 path writes / reads it (hgym_net_shadow_ld returns 0 otherwise). */
typedef struct HgymObsShadow {
    void* obs;       /* (M, ld_obs) bf16 */
    int64_t ld_obs;
    void* priv;      /* (M, ld_priv) bf16 */
    int64_t ld_priv;
} HgymObsShadow;
/* leading dimension (elements) of the bf16 shadow of net `which`'s input rows (0 actor: obs, 1 critic: privileged obs), or 0 when
 * this configuration does not take the fused bf16 path */
int64_t hgym_net_shadow_ld(const HgymNetConfig* cfg, int32_t which);
/* The critic over M stored privileged-observation rows in one call (ActorCritic.evaluate, actor_critic.py:127-129, on every slot of a
 * finished rollout): values (M,) fp32; shadow->priv (optional) receives the bf16 of the rows, as the per-step policy launches leave it.
 * M may exceed HgymNetConfig.max_batch (the rows are walked in pieces). */
int32_t hgym_critic_values(const HgymNetConfig* cfg, const HgymNet* net, int64_t M, const float* priv, float* values,
                           const HgymObsShadow* shadow, void* stream);

/* PPO.act (ppo.py:91-101): mu = actor(obs); sigma = std; a = mu + sigma*z; V = critic(priv);
 * logp = sum log N(a; mu, sigma).  (HGYM_STD_LOG: std = exp(log_std), read from the derived block; the `sigma` output is sigma itself.)  z (M,12) standard normal draws or NULL -> Philox(seed, *step_counter).
 * Outputs row-major: actions/mu/sigma (M,12), logp (M,), values (M,). */
int32_t hgym_policy_act(const HgymNetConfig* cfg, const HgymNet* net, int32_t M, const float* obs,
                        const float* priv, const float* z, uint64_t seed, const int64_t* step_counter,
                        float* actions, float* mu, float* sigma, float* logp, float* values,
                        const HgymObsShadow* shadow, void* stream);

/* hgym_policy_act + the postponed step finaliser of the PREVIOUS env step (env_cfg / env_st / env_out as that step got them,
 * env_out->defer_finalize = 1) as one extra workgroup of the same launch: one launch less per vec-step. */
int32_t hgym_policy_act_fin(const HgymNetConfig* cfg, const HgymNet* net, int32_t M, const float* obs,
                            const float* priv, const float* z, uint64_t seed, const int64_t* step_counter,
                            float* actions, float* mu, float* sigma, float* logp, float* values,
                            const HgymEnvConfig* env_cfg, const HgymEnvState* env_st, const HgymEnvOut* env_out,
                            const HgymObsShadow* shadow, void* stream);

/* Temporally correlated exploration noise (added within header v9, no layout change): the `z` tables of all T policy launches of a
 * rollout in ONE launch ahead of it.  For env m, action j and t = 0 .. T-1
 *     z[t][m][j] = carry[t] * state[m][j] + sum_{s = 0 .. t} filt[t * ld_filt + s] * w_s[m][j]
 * where w_s[m][j] is, bit for bit, the standard normal hgym_policy_act (z = NULL, this seed) draws for (m, j) when *step_counter holds
 * *step + s: the same key, the same counter words, slot 64 + j / 4, the same Box-Muller pairing.  fp32: the carry term first (+0 without
 * one), then s ascending, every multiply and every add rounded on its own.  Only the lower triangle of filt is read.
 * z (T, n, A) row-major: row t is the `z` argument of the policy launch of step *step + t (hgym_policy_act, hgym_policy_act_fin,
 * hgym_rollout_step_z).  carry: T floats or NULL.  state (n, A): read, then overwritten with z[T-1] (the process continues across calls:
 * AR(1) with filt[t][s] = sqrt(1 - r^2) r^(t-s), carry[t] = r^(t+1)); NULL allowed only with carry NULL, and then not written.
 * step: a device int64, read by the launch (fixed arguments: capturable).  With filt the identity and no carry the table is the draws
 * themselves.  Stores are 16 bytes wide where A % 4 == 0 and z is 16-byte aligned.
 * Nothing launched and HGYM_E_SHAPE: T outside [1, HGYM_NOISE_MAX_STEPS], A outside [1, 12], n < 1, ld_filt < T.  HGYM_E_BADARG: a NULL
 * filt, step or z; a carry with state NULL; a float pointer not 4-byte aligned, step not 8-byte.  HGYM_E_UNSUPPORTED: n >= 2^31. */
#define HGYM_NOISE_MAX_STEPS 128
int32_t hgym_policy_noise_table(int32_t T, int64_t n, int32_t A, const float* filt, int64_t ld_filt, const float* carry, float* state,
                                uint64_t seed, const int64_t* step, float* z, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused rollout step: PPO.act + XBotLFreeEnv.step (synthetic-physics backend) + the previous step's finaliser in ONE launch
 * (algo/ppo/on_policy_runner.py:129-141 is the loop body this stands for: act -> env.step -> process_env_step).
 * Workgroup b computes the actor tile of envs [32 b, 32 b + 32), samples their actions and runs their env step right behind it;
 * a second grid row holds the critic tiles, a third the finaliser of the PREVIOUS step (HgymEnvOut.defer_finalize semantics:
 * the transition sink of `prev_out`, extras, counters).  Results are those of hgym_policy_act_fin followed by
 * hgym_env_step_synth: same kernels' source, same arithmetic.
 *
 * Calling sequence for a rollout of T steps, parity(t) alternating 0 / 1:
 *     hgym_rollout_begin(st, step_counter, scratch, parity(0))
 *     for t in 0..T-1:  hgym_rollout_step(..., out[t], t ? out[t-1] : NULL, obs[t], priv[t], ..., scratch, parity(t))
 *     hgym_rollout_end(env_cfg, st, out[T-1], scratch, parity(T-1))
 * where out[t] has obs / priv_obs = where the observations of step t+1 go, the transition sink of step t (t_values = the
 * `values` buffer of the same call, t_rewards / t_dones, t_step = step_counter), defer_finalize = 1, and -- because the
 * finaliser of step t-1 runs concurrently with the env phase of step t -- rew / reset / time_out buffers DISTINCT from
 * out[t-1]'s (two sets, alternating).  Between begin and end no other env entry point may run on this state.
 * scratch: HGYM_ROLLOUT_SCRATCH_BYTES(num_envs) bytes owned by the caller, 16-byte aligned, zero-filled once (ping-pong step
 * counters, per-parity reset count and episode-sum accumulators; behind that header the env step's draw tables, which the
 * critic workgroups of step t compute for step t + 1).  Supported: the XBot-L default options (none of the generic ones, no use_ref_actions),
 * 15 / 3 history, contiguous [136][N] state, SoA sim tensors, N a multiple of 32, the bf16 fused net path (so activation ELU(1));
 * HGYM_E_UNSUPPORTED otherwise (callers fall back to hgym_policy_act_fin + hgym_env_step_synth).
 * values = NULL (header v7, deferred values): no critic tiles -- the grid is the N / 32 actor + env workgroups and the finaliser, every
 * workgroup draws its own step's random numbers and copies its own history rows (the critic workgroups' side jobs), and the
 * sinks of out / prev_out must be of the deferred kind (t_values NULL, t_time_outs set); obs_ahead / obs_older_ready / l0_* stay
 * NULL / 0; `priv` is not read and the shadow's priv member is not written (hgym_critic_values does both after the rollout).  This is
 * the form for more than half a chip of envs (N / 32 > CUs / 2: 8192 envs per MI355X), where the critic's tiles would need the
 * compute units of a second round.
 * ---------------------------------------------------------------------------------------------- */
#define HGYM_ROLLOUT_SCRATCH_HEADER_BYTES 512
#define HGYM_ROLLOUT_DRAW_BYTES_PER_ENV 1000      /* two parities x 125 floats */
#define HGYM_ROLLOUT_SCRATCH_BYTES(num_envs) (HGYM_ROLLOUT_SCRATCH_HEADER_BYTES + (size_t)HGYM_ROLLOUT_DRAW_BYTES_PER_ENV * (size_t)(num_envs))
int32_t hgym_rollout_begin(const HgymEnvState* st, const int64_t* step_counter, void* scratch, int32_t parity, void* stream);
int32_t hgym_rollout_step(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                          const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs,
                          const float* priv, uint64_t seed, float* actions, float* mu, float* sigma, float* logp, float* values,
                          void* scratch, int32_t parity, const HgymObsShadow* shadow, void* stream);
/* hgym_rollout_step with this step's normals handed in (added within header v9): z (num_envs, 12) fp32, 4-byte aligned -- a row of
 * hgym_policy_noise_table's table -- replaces the actor epilogue's own Philox draw, as the `z` of hgym_policy_act does; `seed` and the
 * scratch block's sampling step are then not used by the sampling.  The same kernels, the same launches.  z = NULL: hgym_rollout_step. */
int32_t hgym_rollout_step_z(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                            const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs,
                            const float* priv, uint64_t seed, float* actions, float* mu, float* sigma, float* logp, float* values,
                            void* scratch, int32_t parity, const HgymObsShadow* shadow, void* stream, const float* z);
int32_t hgym_rollout_end(const HgymEnvConfig* env_cfg, const HgymEnvState* st, const HgymEnvOut* last_out, void* scratch,
                         int32_t parity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation rollout (header v9, no layout change): the policy's MEAN action instead of a sample, what scripts/play.py and an
 * exported policy run (ActorCritic.act_inference, actor_critic.py:122-124, followed by VecEnv.step).
 *
 * hgym_rollout_eval_step is the values = NULL form of hgym_rollout_step without everything that serves training: workgroup b computes
 * the actor tile of envs [32 b, 32 b + 32) and runs their env step on action = mu right behind it; a second grid row carries the
 * finaliser of the PREVIOUS step (prev_out; NULL on the first step).  No Philox draw for the policy, no sigma, no log-probability, no
 * critic tile, no storage slot, no bf16 shadow, no transition sink.  `actions` (N, 12) receives mu: bit for bit what hgym_policy_act
 * returns as `mu` for the same rows, and the env step is that of hgym_env_step_synth on those actions.
 * Calling sequence for T steps, parity(t) alternating: hgym_rollout_begin(st, any device int64, scratch, parity(0)); T calls with
 * out[t].obs / priv_obs = where the observations of step t + 1 go (not the rows the call reads), the sinks NULL, defer_finalize = 1,
 * rew / reset / time_out distinct from out[t-1]'s; hgym_rollout_end(env_cfg, st, out[T-1], scratch, parity(T-1)).  Same scratch block,
 * same restrictions as hgym_rollout_step (HGYM_E_UNSUPPORTED otherwise; callers fall back to hgym_mlp_forward + hgym_env_step_synth),
 * except that nothing is asked of the critic.
 * ---------------------------------------------------------------------------------------------- */
int32_t hgym_rollout_eval_step(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                               const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs,
                               float* actions, void* scratch, int32_t parity, void* stream);

/* The evaluation accumulator: one caller-owned block of HGYM_EVAL_BLOCK_DOUBLES(n) doubles, zeroed by hgym_eval_reset, added to by one
 * hgym_eval_accumulate behind every vec-step (fused or not: it reads the env state and the step's outputs as any env step leaves them),
 * read back once.  fp64 sums formed in a fixed order (per-workgroup partials, added by the last workgroup to arrive): the same
 * trajectory gives the same bits.  Totals, block[HGYM_EVAL_*]:
 *   STEPS       vec-steps seen                       ENV_STEPS   env-steps seen (n per vec-step)
 *   LIN_ERR     sum of |commands[:, :2] - base_lin_vel[:, :2]|_2        ANG_ERR   sum of |commands[:, 2] - base_ang_vel[:, 2]|
 *   REWARD      sum of rew
 *   EPISODES    envs with reset set                  TIMEOUTS    ... of which time_out was set
 *   RETURN      sum over finished episodes of their return (sum of rew since the env's previous reset, or since hgym_eval_reset)
 *   LENGTH      ... of their length in steps
 *   TERMS + k   ... of HgymEnvState.episode_sums[k] as it stood BEFORE the episode's last step: the env step consumes and zeroes the
 *               finished sums inside its launch, so the accumulator credits the copy it took one step earlier (k in the order of
 *               HgymEnvConfig.reward_scales; the last step's terms are missing from these 22 sums, not from RETURN)
 * The velocity errors compare the command and the base velocity as the step leaves them (for an env that has just reset: its new
 * command and its reset velocity).  Behind the totals the block holds the per-workgroup partials and the per-env running return,
 * length and copy of the episode sums.  commands / base_lin_vel / base_ang_vel / episode_sums: the [C][n] arrays of HgymEnvState;
 * rew / reset / time_out: that step's HgymEnvOut buffers. */
#define HGYM_EVAL_SUMS 32
#define HGYM_EVAL_STEPS 0
#define HGYM_EVAL_ENV_STEPS 1
#define HGYM_EVAL_LIN_ERR 2
#define HGYM_EVAL_ANG_ERR 3
#define HGYM_EVAL_REWARD 4
#define HGYM_EVAL_EPISODES 5
#define HGYM_EVAL_TIMEOUTS 6
#define HGYM_EVAL_RETURN 7
#define HGYM_EVAL_LENGTH 8
#define HGYM_EVAL_TICKET 9      /* arrival counter of the running call (an integer in the slot's first word; zero between calls) */
#define HGYM_EVAL_TERMS 10      /* 22 slots */
#define HGYM_EVAL_ENVS_PER_PARTIAL 256
#define HGYM_EVAL_BLOCK_DOUBLES(n) ((size_t)HGYM_EVAL_SUMS * (1 + ((size_t)(n) + HGYM_EVAL_ENVS_PER_PARTIAL - 1) / HGYM_EVAL_ENVS_PER_PARTIAL) + \
                                    (size_t)(2 + HGYM_NUM_REWARDS) * (size_t)(n))
int32_t hgym_eval_reset(int32_t n, double* block, void* stream);
int32_t hgym_eval_accumulate(int32_t n, const float* commands, const float* base_lin_vel, const float* base_ang_vel,
                             const float* episode_sums, const float* rew, const uint8_t* reset, const uint8_t* time_out, double* block,
                             void* stream);

/* One minibatch of PPO.update up to and including backward (ppo.py:128-171), device side only:
 * gathers rows `idx[0..B)` (indices into the flattened (T*N) storage, rollout_storage.py:151-182) of the
 * nine storage tensors, forward, KL -> learning-rate adaptation (written to opt_state[HGYM_OPT_LR]), clipped
 * surrogate + clipped value loss + entropy bonus, hand-written backward -> net->grads (un-clipped). */
typedef struct HgymBatch {
    const float* obs;        /* (T*N, num_obs)   */
    const float* priv;       /* (T*N, num_priv)  */
    const float* actions;    /* (T*N, 12) */
    const float* values;     /* (T*N,)    */
    const float* advantages; /* (T*N,)    */
    const float* returns;    /* (T*N,)    */
    const float* logp;       /* (T*N,)    */
    const float* mu;         /* (T*N, 12) */
    const float* sigma;      /* (T*N, 12) */
    const int64_t* idx;      /* (B,) */
    int32_t B;
    /* optional bf16 shadows of obs / priv, same rows (HgymObsShadow: written by the policy launches that read those rows), leading
     * dimensions hgym_net_shadow_ld(cfg, 0 / 1); both or neither.  NULL: the fp32 rows are gathered and converted (and a bf16
     * operand copy of the gathered rows is kept for the weight-gradient kernel). */
    const void* obs_bf16;
    const void* priv_bf16;
    int64_t num_rows;        /* rows of the storage tensors (T*N), required (> 0) with the shadows: the weight-gradient kernel addresses a
                                shadow with 32-bit byte offsets, so num_rows * hgym_net_shadow_ld(cfg, 0) * 2 must stay below 4 GiB (2.79 M
                                rows for XBot-L) -- beyond that the fp32 rows are used */
    /* the mirror loss (HgymPPOConfig.mirror_coef > 0; ignored at 0; appended within header v9: a zero-filled tail with mirror_coef = 0 is
     * a batch of any earlier layout).  With mirror_coef > 0 any of the five NULL, or mirror_target not 16-byte aligned: HGYM_E_BADARG and
     * nothing launched.  pair_idx, mirror_act_src and mirror_act_sign are DEVICE arrays read by the launches: the library cannot
     * validate their contents without a host synchronisation (the Python layer does: MirrorSpec, mirror_pair_rows); an act_src entry
     * outside [0, num_actions) is clamped into it. */
    const int64_t* pair_idx;        /* (B,) the partner's storage row of every row of idx */
    const int32_t* mirror_act_src;  /* (num_actions,) M_a's source column */
    const float* mirror_act_sign;   /* (num_actions,) M_a's sign */
    float* mirror_target;           /* caller-owned scratch, (B, num_actions) fp32, 16-byte aligned: receives the RAW mu(obs[pair_idx]) (M_a is
                                       applied where the loss reads it) */
    double* mirror_sums;            /* two device doubles the caller zeroes: [0] += this minibatch's L_m / mirror_coef (the plain MSE),
                                       [1] += 1 */
} HgymBatch;

int32_t hgym_ppo_grad(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net,
                      const HgymBatch* batch, void* stream);

/* hgym_ppo_grad in two halves (one process per GPU; the reference is single-process, its `--horovod` flag is dead:
 * utils/helpers.py:207-212), for a caller that wants to start exchanging the first gradient bucket a few microseconds early:
 *   part 0: forward, loss, dZ chain and ALL weight-gradient products (of every net, the auxiliary head included), then the slab
 *           sums of [std | actor]: on return (stream order) grads[0 .. hgym_net_param_offset(cfg, 1)) -- 527 256 of 926 106
 *           floats -- are final;
 *   part 1: the slab sums of the rest: grads[hgym_net_param_offset(cfg, 1) .. P] -- critic | auxiliary head | the KL slot.
 * (Until round 3 part 1 also launched the critic's weight-gradient products on their own, so that the first bucket travelled
 * under them: two launches of 144 and 112 workgroups on 256 CUs took 2 x 142 us against 178 us for the one launch, more than the
 * exchange they hid.  PPO.update now calls hgym_ppo_grad and exchanges ONE bucket.)
 * part 0 followed by part 1 leaves net->grads exactly as hgym_ppo_grad does (bit-identical), and opt_state[HGYM_OPT_GRAD_SQNORM] (the squared norm
 * hgym_ppo_apply may reuse with grad_norm_ready) complete: part 0 zeroes it and adds its bucket's share, part 1 adds the rest.
 * Between part 0 and part 1 it is partial; with world_size > 1 apply recomputes the norm of the rank mean regardless. */
int32_t hgym_ppo_grad_part(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net,
                           const HgymBatch* batch, int32_t part, void* stream);
/* offset (floats) in the flat parameter / gradient vector of the first parameter of net `which` (0 actor, 1 critic, 2 auxiliary
 * head; which == number of nets: the parameter count); -1 on a bad argument */
int64_t hgym_net_param_offset(const HgymNetConfig* cfg, int32_t which);

/* ------------------------------------------------------------------------------------------------
 * Behaviour cloning (header v9, no layout change): one minibatch of rsl_rl's Distillation.update up to and including backward -- the actor
 * regresses its mean on a stored target, nothing else is trained.  With B rows, A actions and e = mu(obs[idx[b]])_j - target[idx[b]][j]:
 *   HGYM_BC_MSE:    L = sum e^2 / (B A),  dL/d mu = 2 e / (B A)                                   (torch's mse_loss)
 *   HGYM_BC_HUBER:  0.5 e^2 where |e| <= delta, else delta (|e| - 0.5 delta), the mean over B A;   (torch's huber_loss)
 *                   dL/d mu = clamp(e, -delta, delta) / (B A)
 * The call reads batch->obs, obs_bf16 (optional: the bf16 shadow of obs, as in hgym_ppo_grad), idx, B and num_rows only; every other
 * member of HgymBatch may be NULL.  target: (num_rows, num_actions) fp32, gathered through idx like obs (16-byte aligned on the fused
 * path).  sums: two device doubles the caller zeroes, [0] += this minibatch's L, [1] += 1.
 * After the call (stream order) net->grads holds: the gradient of L in the actor's weights and biases; exactly +0.0 in the std / log_std
 * slots, the whole critic region, the auxiliary head's region and the KL slot; opt_state[HGYM_OPT_GRAD_SQNORM] the squared norm, as
 * hgym_ppo_grad leaves it.  No other slot of opt_state is touched: no learning-rate decision, no loss sums, no step count.
 * The step is hgym_ppo_apply's, with adaptive_lr = 0 and grad_norm_ready = 0: zero gradient on zero moments moves nothing, so the critic
 * and sigma keep their bits through a whole run of cloning steps.
 * HGYM_E_BADARG before anything is launched: NULL target or sums, loss_type outside {0, 1}, Huber with a delta that is not finite and
 * positive, B < 1 or B > max_batch.  HGYM_E_UNSUPPORTED with HgymNet.norm set. */
#define HGYM_BC_MSE 0
#define HGYM_BC_HUBER 1
typedef struct HgymBCConfig {
    int32_t loss_type;       /* HGYM_BC_MSE / HGYM_BC_HUBER */
    float huber_delta;       /* > 0, finite (read with HGYM_BC_HUBER only) */
} HgymBCConfig;
int32_t hgym_bc_grad(const HgymNetConfig* cfg, const HgymBCConfig* bc, const HgymNet* net, const HgymBatch* batch, const float* target,
                     double* sums, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The smoothness regulariser (header v9, no layout change): a penalty on the policy's mean itself, after CAPS
 * (Mysore et al. 2021).  With B rows, A actions, r_b = idx[b] and mu_b = mu(obs[r_b]) as the update computes it:
 *   temporal   tT_b = mu(obs[next_idx[b]]),                 w_b = next_weight[b]        (hgym_smooth_pairs: r_b + N, 0 where dones[r_b])
 *   spatial    tS_b = mu(obs[r_b] + noise_std (.) z_b),     z_b[c] = normal c of the Philox block at slot 128 (hgym_perturb_rows)
 *   L_s = temporal_coef / (B A) sum_b w_b |mu_b - tT_b|^2 + spatial_coef / (B A) sum_b |mu_b - tS_b|^2
 *   d mu_b += 2 / (B A) (temporal_coef w_b (mu_b - tT_b) + spatial_coef (mu_b - tS_b))
 * Both targets are formed under the current parameters by forward-only passes over fp32 rows: no gradient flows through them.  Nothing
 * but d mu, and hence the actor's gradients, differs from hgym_ppo_grad: d std, the critic, the auxiliary head, the KL slot and the loss
 * sums of opt_state keep their bits.
 *
 * hgym_smooth_pairs: next_idx[b] = idx[b] + N, next_weight[b] = dones[idx[b]] ? 0 : 1 for b in [0, B); one launch, capturable.  The
 *   rollout storage keeps T + 1 observation slots of N rows, so idx[b] + N is always a stored row.
 * hgym_perturb_rows: dst[m][c] = src[row][c] + noise_std[c] * z for m in [0, M), c in [0, width), row = idx ? idx[m] : m; z is normal
 *   number c of the Philox block (key = seed, env word = (uint32) row, step word = (int64) opt_state[HGYM_OPT_STEP] read on the device,
 *   slots 128 .. 128 + ceil(width / 4) - 1), one fused multiply-add.  A column with noise_std[c] == 0 is copied bit for bit.  src rows of
 *   ld_src >= width floats, 4-byte aligned; dst rows of ld_dst floats, ld_dst a multiple of 4 and >= width rounded up to 4, dst 16-byte
 *   aligned.  Columns [width, width rounded up to 4) of dst are written as +0.0, columns behind those are not touched.  One launch,
 *   capturable; HGYM_E_BADARG with nothing launched for a NULL src / noise_std / opt_state / dst, M < 1, width < 1 or a bad leading
 *   dimension / alignment.
 * hgym_ppo_grad_smooth: hgym_ppo_grad with the regulariser.  First of all the spatial pre-pass (hgym_perturb_rows over obs[idx] into
 *   `rows`, the actor's forward over them into target_near; skipped at spatial_coef == 0), then the temporal one (the actor's forward
 *   gathered through next_idx into target_next; skipped at temporal_coef == 0), then hgym_ppo_grad's launches with the actor's loss head
 *   replaced.  The perturbation reads opt_state[HGYM_OPT_STEP] before the call's own loss scalars can advance it.  With both coefficients 0
 *   the launches and the bits are hgym_ppo_grad's.  HGYM_E_BADARG with nothing launched: a negative, NaN or infinite coefficient; a
 *   pointer needed by a term that is on (or sums) NULL; misaligned scratch; ppo->mirror_coef > 0; ppo->world_size > 1. */
typedef struct HgymSmooth {
    float temporal_coef;          /* >= 0, finite; 0: the temporal term is off and next_idx, next_weight, target_next are not read */
    float spatial_coef;           /* >= 0, finite; 0: the spatial term is off and noise_std, seed, target_near, rows are not read */
    const int64_t* next_idx;      /* (B,) the successor's storage row of every row of idx */
    const float* next_weight;     /* (B,) 0 where the row has no successor, else 1 */
    const float* noise_std;       /* (num_obs,) per-column standard deviation of the perturbation, raw observation units */
    uint64_t seed;                /* Philox key of the perturbation */
    float* target_next;           /* caller-owned scratch, (B, num_actions) fp32, 16-byte aligned */
    float* target_near;           /* caller-owned scratch, (B, num_actions) fp32, 16-byte aligned */
    float* rows;                  /* caller-owned scratch, (B, ld) fp32 with ld = num_obs rounded up to 4, 16-byte aligned: receives the
                                     perturbed rows (the padding columns +0.0) */
    double* sums;                 /* four device doubles the caller zeroes: [0] += sum_b w_b |mu_b - tT_b|^2 / (B A), [1] += sum_b |mu_b -
                                     tS_b|^2 / (B A), [2] += sum_b w_b (whenever next_weight is not NULL, either term on), [3] += 1 */
} HgymSmooth;
int32_t hgym_smooth_pairs(int64_t B, int64_t N, const int64_t* idx, const uint8_t* dones, int64_t* next_idx, float* next_weight, void* stream);
int32_t hgym_perturb_rows(int64_t M, int32_t width, const float* src, int64_t ld_src, const int64_t* idx, const float* noise_std, uint64_t seed,
                          const double* opt_state, float* dst, int64_t ld_dst, void* stream);
int32_t hgym_ppo_grad_smooth(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                             const HgymSmooth* smooth, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The mirror loss and the smoothness regulariser in one call (header v9, no layout change).  In the notation of the
 * two terms above, with tm_b the raw mean of the partner row pair_idx[b] and M_a the action table (mirror_act_src, mirror_act_sign),
 * c_m = ppo->mirror_coef, lamT = temporal_coef, lamS = spatial_coef:
 *   L      = L_ppo + c_m / (B A) sum_b |mu_b - M_a tm_b|^2 + lamT / (B A) sum_b w_b |mu_b - tT_b|^2 + lamS / (B A) sum_b |mu_b - tS_b|^2
 *   d mu_b = ((d mu_ppo + g_m (mu_b - M_a tm_b)) + gT w_b (mu_b - tT_b)) + gS (mu_b - tS_b),   g_m = 2 c_m / (B A), gT = 2 lamT / (B A), gS = 2 lamS / (B A)
 * formed in that association, each term by the expression of its own head.  All three targets are formed under the current parameters
 * and detached.  Only d mu, and hence the actor's gradient, differs from hgym_ppo_grad: d std, the critic, the auxiliary head, the KL slot
 * and the loss sums of opt_state keep the bits hgym_ppo_grad gives them on the same inputs.
 *
 * hgym_ppo_grad_smooth_mirror: the launches, in order: the spatial pre-pass (hgym_perturb_rows, then the actor's forward into target_near),
 *   the temporal pre-pass (forward through next_idx into target_next), the mirror pre-pass (forward through batch->pair_idx into
 *   batch->mirror_target), then hgym_ppo_grad's launches with the actor's head replaced.  The perturbation reads opt_state[HGYM_OPT_STEP]
 *   before the call's loss scalars can advance it.  The mirror loss's sums arrive in batch->mirror_sums as from hgym_ppo_grad, the
 *   regulariser's in smooth->sums as from hgym_ppo_grad_smooth: the same bits as the single-option calls give on the same inputs.
 *   head_partials: caller-owned fp32 scratch, 16-byte aligned, head_partials_len >= 4 * ceil(B / 64) floats.  The loss partial row has no
 *   room for the combination's third sum, so the two smoothness errors of every 64-row tile (or 256-row loss block) pass through it; the
 *   caller never reads it.
 *   With ppo->mirror_coef == 0 the call is hgym_ppo_grad_smooth; with both smoothness coefficients 0 it is hgym_ppo_grad, mirror loss
 *   included: the same launches, the same bits, and head_partials is not looked at.
 *   HGYM_E_BADARG with nothing launched: everything hgym_ppo_grad_smooth refuses other than mirror_coef > 0; everything the mirror loss
 *   refuses (a NULL pair_idx, table, mirror_target or mirror_sums, or a misaligned one); with all terms on a NULL, misaligned or too short
 *   head_partials; ppo->world_size > 1.  HgymNet.norm is served as by the two single-option calls. */
int32_t hgym_ppo_grad_smooth_mirror(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                                    const HgymSmooth* smooth, float* head_partials, int64_t head_partials_len, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Guidance by a frozen teacher (header v9, no layout change): a cloning term inside the PPO loss whose coefficient
 * decays (kickstarting, Schmitt et al. 2018, with the squared error of the means in place of a KL).  With B rows, A actions, r_b = idx[b]
 * and mu_b = mu(obs[r_b]) as the update computes it:
 *   t_b   = teacher_mu[r_b]                                  the frozen teacher's mean, formed by the caller for every stored row
 *   c     = *coef                                            one device float, this update's coefficient (hgym_guide_schedule)
 *   L_g   = c / (B A) sum_b sum_j (mu_bj - t_bj)^2
 *   d mu_b += 2 c / (B A) (mu_b - t_b)
 * Nothing but d mu, and hence the actor's gradients, differs from hgym_ppo_grad: d std, the critic, the auxiliary head, the KL slot and the
 * loss sums of opt_state keep their bits.
 *
 * hgym_guide_schedule: one launch of one thread with fixed arguments, capturable.  It reads k = *count, writes
 *   *coef = (float) schedule(k) and then *count = k + 1.  schedule(k), in fp64, left to right, rounded to fp32 once:
 *     HGYM_GUIDE_CONSTANT  coef
 *     HGYM_GUIDE_STEP      k < final_step ? coef : final_value
 *     HGYM_GUIDE_LINEAR    k <= initial_step ? coef : k >= final_step ? final_value
 *                          : coef + (final_value - coef) * (double)(k - initial_step) / (double)(final_step - initial_step)
 *   HGYM_E_BADARG with nothing launched: a NULL or misaligned pointer (count 8 bytes, coef 4), an unknown mode, a negative, NaN or
 *   infinite coef / final_value, a negative step, LINEAR with final_step <= initial_step.
 * hgym_ppo_grad_guide: hgym_ppo_grad's launches with the actor's loss head replaced (fused path: the actor's tiles through kernels of
 *   their own, which stage the tile's 64 target rows in LDS where there is room; layer-by-layer path: one kernel behind the loss head),
 *   then one workgroup that adds the per-tile squared errors in a fixed order.  The coefficient is read from the device by the head, so
 *   a captured call follows a coefficient that changes.  With *coef == 0.0 every gradient has hgym_ppo_grad's value.
 *   HGYM_E_BADARG with nothing launched: a NULL guide, teacher_mu, coef or sums; teacher_mu not 16-byte aligned (coef 4, sums 8);
 *   ppo->mirror_coef > 0 (separate heads); ppo->world_size > 1.  HgymNet.norm is served as by hgym_ppo_grad. */
#define HGYM_GUIDE_CONSTANT 0
#define HGYM_GUIDE_STEP 1
#define HGYM_GUIDE_LINEAR 2
typedef struct HgymGuideSchedule {
    double coef;              /* >= 0, finite: the coefficient up to initial_step (LINEAR), below final_step (STEP), always (CONSTANT) */
    double final_value;       /* >= 0, finite: the coefficient from final_step on (STEP, LINEAR) */
    int64_t initial_step;     /* LINEAR: the last update count at `coef` */
    int64_t final_step;       /* STEP, LINEAR: the first update count at final_value */
    int32_t mode;             /* HGYM_GUIDE_CONSTANT / HGYM_GUIDE_STEP / HGYM_GUIDE_LINEAR */
    int32_t reserved;         /* 0 */
} HgymGuideSchedule;
typedef struct HgymGuide {
    const float* teacher_mu;  /* (batch->num_rows, num_actions) fp32, 16-byte aligned: the teacher's mean of every stored row, gathered
                                 through batch->idx like every other loss input */
    const float* coef;        /* one device float: this update's coefficient, >= 0 */
    double* sums;             /* two device doubles the caller zeroes: [0] += sum_b |mu_b - t_b|^2 / (B A), [1] += 1 */
} HgymGuide;
int32_t hgym_guide_schedule(const HgymGuideSchedule* sched, int64_t* count, float* coef, void* stream);
int32_t hgym_ppo_grad_guide(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                            const HgymGuide* guide, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diagnostics of an update (header v9, no layout change): what the update did to the policy, measured on the rows it trained on.
 * The reference logs none of this (ppo.py:176-184 returns the two mean losses); the per-row forms are those of its loss (ppo.py:128-166).
 *
 * hgym_ppo_diag_reduce is the reduction alone over M rows: actions / mu_old / sigma_old / mu_new (M, 12) fp32 row-major, 16-byte
 * aligned; logp_old / values_old / returns / advantages / values_new (M,) fp32; std = the 12 current standard deviations (the head of
 * HgymNet.params; with HGYM_STD_LOG the derived block at hgym_net_sigma_offset, NOT the parameters: `std` is always sigma, never its
 * logarithm -- hgym_ppo_diagnostics passes the right one itself).  Per row, in fp32:
 *     logp_new  = sum_j -(a_j - mu_new_j)^2 / (2 std_j^2) - log std_j - log sqrt(2 pi)       ratio = expf(logp_new - logp_old)
 *     kl        = sum_j log(std_j / sigma_old_j) + (sigma_old_j^2 + (mu_old_j - mu_new_j)^2) / (2 std_j^2) - 1/2     (old || new, exact;
 *                 the learning-rate rule's expression, ppo.py:138-139, has + 1e-5 inside the logarithm: 1.2e-4 for a policy that did
 *                 not move at all, so its sum in opt_state[HGYM_OPT_KL_SUM] lies that much above this one)
 *     surrogate = max(-A ratio, -A clamp(ratio, 1 - clip, 1 + clip))                         entropy = sum_j 1/2 + log sqrt(2 pi) + log std_j
 * and, widened to fp64, combined into block[HGYM_DIAG_*]:
 *   COUNT          rows                                   KL           sum kl
 *   APPROX_KL      sum (ratio - 1) - (logp_new - logp_old)             RATIO        sum ratio
 *   CLIPPED        rows with ratio < 1 - clip or ratio > 1 + clip (the bounds formed in fp32, as torch.clamp gets them)
 *   RATIO_MAX, RATIO_MIN    over all rows (-inf, +inf without rows)    SURROGATE    sum surrogate
 *   RET, RET_SQ    sum R, sum R^2                         ERR_OLD, ERR_OLD_SQ   sum (R - V_old), sum (R - V_old)^2
 *   ERR_NEW, ERR_NEW_SQ     the same with V_new           VALUE_CLIPPED         rows with |V_new - V_old| > clip
 *   ENTROPY        sum entropy
 * Order of summation: one partial per 256 GLOBAL rows -- rows [row0, row0 + M) of total_rows fill slots row0 / 256 ... of the block --
 * formed by a fixed tree over lanes, then wavefronts; the call with finish = 1 then combines the partials of rows [0, row0 + M) in slot
 * order and WRITES the totals.  The same rows give the same bits in every run, reduced by one call or by several; no atomics.
 * row0 must be a multiple of 256, and so must M in every call but the last (finish = 1); M = 0 with finish = 1 is legal; rows beyond
 * total_rows (what the block was sized for) are refused: all HGYM_E_BADARG, and nothing is launched.
 * block: HGYM_DIAG_BLOCK_DOUBLES(total_rows) doubles of the caller, zeroed by hgym_ppo_diag_reset (the totals, then 16 per partial).
 *
 * hgym_ppo_diagnostics is the whole pass over the M rows `rows` points to (an HgymBatch whose idx is not read -- the rows are taken in
 * order; B, the shadows and num_rows are ignored): in pieces of at most cfg->max_batch rows rounded down to a multiple of 256 (M <=
 * max_batch: one piece), the actor forward (hgym_mlp_forward, which = 0) and the critic forward (hgym_critic_values, no shadow) of
 * the piece into `scratch` (max_batch x 13 floats, 16-byte aligned: mu_new, then values_new), then hgym_ppo_diag_reduce on it with
 * clip = ppo->clip_param, finish on the last piece.  The block equals, bit for bit, what those three calls give when the caller makes
 * them.  Allocates nothing, synchronises nothing; reads the parameters and writes only scratch, block and the forwards' workspace:
 * opt_state, the gradients, the Adam moments and the observation shadows are not touched.  Legal between hgym_ppo_apply and the next
 * rollout launch on the same stream.  M > max_batch with max_batch < 256: HGYM_E_SHAPE. */
#define HGYM_DIAG_SUMS 16
#define HGYM_DIAG_COUNT 0
#define HGYM_DIAG_KL 1
#define HGYM_DIAG_APPROX_KL 2
#define HGYM_DIAG_RATIO 3
#define HGYM_DIAG_CLIPPED 4
#define HGYM_DIAG_RATIO_MAX 5
#define HGYM_DIAG_RATIO_MIN 6
#define HGYM_DIAG_SURROGATE 7
#define HGYM_DIAG_RET 8
#define HGYM_DIAG_RET_SQ 9
#define HGYM_DIAG_ERR_OLD 10
#define HGYM_DIAG_ERR_OLD_SQ 11
#define HGYM_DIAG_ERR_NEW 12
#define HGYM_DIAG_ERR_NEW_SQ 13
#define HGYM_DIAG_VALUE_CLIPPED 14
#define HGYM_DIAG_ENTROPY 15
#define HGYM_DIAG_ROWS_PER_PARTIAL 256
#define HGYM_DIAG_MAX_ROWS 2147483648      /* 2^31: partial slots and launch grids stay 32-bit */
#define HGYM_DIAG_BLOCK_DOUBLES(total_rows) \
    ((size_t)HGYM_DIAG_SUMS * (1 + ((size_t)(total_rows) + HGYM_DIAG_ROWS_PER_PARTIAL - 1) / HGYM_DIAG_ROWS_PER_PARTIAL))
int32_t hgym_ppo_diag_reset(int64_t total_rows, double* block, void* stream);
int32_t hgym_ppo_diag_reduce(int64_t M, const float* actions, const float* mu_old, const float* sigma_old, const float* mu_new,
                             const float* logp_old, const float* values_old, const float* returns, const float* advantages,
                             const float* values_new, const float* std, float clip_param, int64_t row0, int64_t total_rows, int32_t finish,
                             double* block, void* stream);
int32_t hgym_ppo_diagnostics(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* rows, int64_t M,
                             float* scratch, double* block, void* stream);

/* clip_grad_norm_ + Adam.step (ppo.py:173-174) on net->grads (the rank-SUM when world_size > 1: divided by
 * world_size here, as is the KL in grads[P] before the learning-rate decision), refreshes the
 * compute-precision shadows, bumps opt_state. */
int32_t hgym_ppo_apply(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Critic only (header v9, no layout change): one minibatch of the value part of PPO.update up to and including
 * backward -- the critic regresses on the stored returns, nothing else is trained.  With B rows, r_b = idx[b], v_b = V(priv[r_b]),
 * R_b = returns[r_b], vold_b = values[r_b], c = clip_param:
 *   clipped:    vc_b = vold_b + clamp(v_b - vold_b, -c, c),  L = sum_b max((v_b - R_b)^2, (vc_b - R_b)^2) / B   (ties of the max split evenly,
 *               the clamp passes gradient on the closed range: torch's backward, as in hgym_ppo_grad)
 *   unclipped:  L = sum_b (v_b - R_b)^2 / B                                              (HgymPPOConfig.value_loss_unclipped's form)
 *   d v_b = value_coef / B * dL_b/dv_b: value_coef multiplies the gradient, not the reported loss.
 * hgym_vf_grad reads batch->priv, priv_bf16 (optional: the bf16 shadow of priv, as in hgym_ppo_grad; 16-byte aligned), values (clipped
 * form only), returns, idx, B and num_rows; every other member of HgymBatch may be NULL.  sums: two device doubles the caller zeroes,
 * [0] += this minibatch's L, [1] += 1.
 * After the call (stream order) net->grads holds the gradient of value_coef * L in the critic's weights and biases.  On the fused bf16
 * path the critic's tiles, the weight-gradient products and the slab sums are the kernels hgym_ppo_grad runs for the critic: the critic
 * region has that call's bits on the same inputs.  keep_others = 0: every other slot -- std / log_std, the actor, the auxiliary head, the
 * KL slot -- is exactly +0.0 and opt_state[HGYM_OPT_GRAD_SQNORM] is SET to the critic's squared norm.  keep_others = 1: those slots are not
 * touched and the critic's squared norm is ADDED to opt_state[HGYM_OPT_GRAD_SQNORM].  No other slot of opt_state is touched: no
 * learning-rate decision, no loss sums, no step count.  The step is hgym_ppo_apply's, with adaptive_lr = 0 and grad_norm_ready = 0: zero
 * gradient on zero moments moves nothing, so the actor and sigma keep their bits while their Adam moments are zero.
 * HgymNet.norm is served as by hgym_ppo_grad (hgym_net_norm_unfold_grad follows, as there).  One rank.
 * HGYM_E_BADARG before anything is launched: a NULL cfg, vf, net, batch or sums (sums 8-byte aligned); unclipped or keep_others outside
 * {0, 1}; value_coef, or clip_param with the clipped form, negative, NaN or infinite; B < 1 or B > max_batch; NULL priv, returns or idx, or
 * NULL values with the clipped form; a misaligned shadow.
 *
 * hgym_bc_vf_grad: a cloning step that also trains the critic.  net->grads, opt_state[HGYM_OPT_GRAD_SQNORM], bc_sums and vf_sums equal, bit
 * for bit, hgym_bc_grad followed by hgym_vf_grad with keep_others = 1 (which vf->keep_others is ignored for) on the same inputs; the
 * launches are fewer: the actor's tiles with the regression head, the critic's plain tiles, ONE weight-gradient launch with all
 * products (every product is summed by workgroups of its own, whatever shares the launch), one slab pass, one scalars workgroup.
 * Refuses what either of the two refuses. */
typedef struct HgymVFConfig {
    float clip_param;     /* value clip range (read unless unclipped) */
    float value_coef;     /* multiplies the gradient, not the reported loss */
    int32_t unclipped;    /* 1: (R - V)^2, as HgymPPOConfig.value_loss_unclipped */
    int32_t keep_others;  /* 0: every gradient slot outside the critic's region becomes +0.0 and
                             opt_state[HGYM_OPT_GRAD_SQNORM] is SET to the critic's squared norm;
                             1: those slots are left as found and the critic's squared norm is ADDED */
} HgymVFConfig;
int32_t hgym_vf_grad(const HgymNetConfig* cfg, const HgymVFConfig* vf, const HgymNet* net, const HgymBatch* batch, double* sums,
                     void* stream);
int32_t hgym_bc_vf_grad(const HgymNetConfig* cfg, const HgymBCConfig* bc, const HgymVFConfig* vf, const HgymNet* net,
                        const HgymBatch* batch, const float* target, double* bc_sums, double* vf_sums, void* stream);

/* ---- direct gradient exchange over peer mappings (header v6 / v7; the alternative to the RCCL all-reduce of the data-parallel update
 * that HGYM_COMM=auto probes and picks at start-up:
 * reference has nothing here, /root/reference/humanoid/utils/helpers.py:207-212 is a dead flag).  One process per GPU.  Every rank
 * allocates ONE fine-grained buffer with hgym_comm_alloc, exports its handle (hgym_comm_ipc_export, 64 bytes, exchanged by the
 * caller over whatever it has -- torch.distributed's all_gather_object here), opens the peers' (hgym_comm_ipc_open) and fills an
 * HgymComm: data[q] = rank q's payload (count floats, count % 4 == 0; data[rank] is the caller's own -- the flat [gradient | KL] vector
 * lives there, HgymNet.grads points into it), flags[q] = rank q's flag block (HGYM_COMM_FLAG_WORDS zero-filled uint32), status = 16
 * int64 of the caller's own buffer.  hgym_comm_allreduce(seq = 1, 2, 3, ... -- the same sequence on every rank; or 0, below) enqueues ONE kernel that
 * leaves the rank-ordered fp32 SUM in every rank's data (bit-identical on all ranks): arrival flags, each rank sums its 1 / world shard
 * from all buffers and stores the result into all buffers, completion flags.  Waits are bounded (wait_ticks of the 100 MHz wall clock,
 * 0 = 15 s): on expiry status[0] = 1 (sticky until the caller clears it), status[1] = the seq of the call, that call's payload is
 * garbage and the communicator stays usable for later calls.  hgym_comm_status synchronises `stream` and copies the 16 status words
 * to the host: call it where the host synchronises anyway.  status[8 .. 10] = 100 MHz timestamps of the last call: start, every
 * rank arrived, every shard delivered. */
#define HGYM_COMM_MAX_RANKS 8
#define HGYM_IPC_HANDLE_BYTES 64
#define HGYM_COMM_FLAG_WORDS 32
typedef struct HgymComm {
    int32_t world, rank;
    float* data[HGYM_COMM_MAX_RANKS];
    uint32_t* flags[HGYM_COMM_MAX_RANKS];
    int64_t count;
    int64_t* status;
    int64_t wait_ticks;     /* v7: bound of every wait inside hgym_comm_allreduce, 100 MHz ticks; 0 = the default (15 s) */
    double* aux[HGYM_COMM_MAX_RANKS];   /* v9: aux[q] = rank q's block of HGYM_COMM_AUX_DOUBLES zero-filled doubles in the same fine-grained
                                         * allocation (hgym_comm_sum64's slots); NULL everywhere if hgym_comm_sum64 is not used */
} HgymComm;
int32_t hgym_comm_alloc(int64_t bytes, void** dev_ptr);
int32_t hgym_comm_free(void* dev_ptr);
int32_t hgym_comm_ipc_export(void* dev_ptr, void* handle_out);
int32_t hgym_comm_ipc_open(const void* handle, void** dev_ptr);
int32_t hgym_comm_ipc_close(void* dev_ptr);
int32_t hgym_comm_allreduce(const HgymComm* comm, uint32_t seq, void* stream);
/* header v9 -- what lets a data-parallel update be captured into a HIP graph (no launch argument changes from call to call, no
 * torch.distributed call inside):
 *   hgym_comm_allreduce(seq = 0): the call number is kept on the device -- status[2] = number of the last call, read by the kernel on
 *   entry and advanced by it; all ranks must use the same form for the same call (a communicator is driven either with explicit numbers
 *   or with 0 throughout);
 *   hgym_comm_sum64: in-place SUM over the ranks of n <= 3 doubles at `vals` (device memory of the caller) -- the per-iteration
 *   (sum adv, sum adv^2, count) of RolloutStorage.compute_returns' normalisation (rollout_storage.py:132-136 over the global batch) --
 *   through aux[]: one wavefront, tagged slots, summed in rank order (bit-identical on all ranks); its call number is status[3];
 *   bounded waits as above (status[0] = 1 on expiry). */
#define HGYM_COMM_AUX_DOUBLES (2 * HGYM_COMM_MAX_RANKS * 4)
int32_t hgym_comm_sum64(const HgymComm* comm, double* vals, int32_t n, void* stream);
int32_t hgym_comm_status(const HgymComm* comm, int64_t* host16, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py's roofline leg).  PROCESS-GLOBAL state, unlike the rest of this interface: one event list and one
 * phase buffer per process, not per device or per stream, and not thread-safe -- enable them from one thread, for one device at
 * a time.  (Everything else keeps no state between calls except the per-(kernel, device) record of how much dynamic LDS has been
 * reserved, which is mutex-guarded: one process may drive several devices and streams.)  When enabled, every launch of a profiled kernel class is
 * bracketed by a pair of HIP events recorded on the launch stream; the summary synchronises those events and
 * returns launches, summed duration and summed ALGORITHMIC work (flops for the GEMM class, bytes for the
 * HBM-bound classes; DESIGN.md states the per-unit figures).  Off by default; not capturable in a hipGraph.
 * ---------------------------------------------------------------------------------------------- */
enum {
    HGYM_PROF_GEMM = 0,      /* generic MFMA GEMM launches (fp32 parity path / unsupported layer shapes) */
    HGYM_PROF_ENV_STEP = 1, HGYM_PROF_GAE = 2, HGYM_PROF_LOSS = 3,
    HGYM_PROF_MLP_FWD = 4,   /* the update's fused forward + loss + dZ chain (64-row tiles, writes the activations and their gradients) */
    HGYM_PROF_MLP_BWD = 5,   /* (unused since the dZ chain runs inside the class-4 kernel; the value is kept) */
    HGYM_PROF_DW = 6,        /* all weight-gradient products */
    HGYM_PROF_REDUCE = 7,    /* split-K slab reduction */
    HGYM_PROF_APPLY = 8,     /* grad-norm + clip + Adam */
    HGYM_PROF_POLICY = 9,    /* fused forward, rollout / inference (32-row tiles, sampling epilogue) */
    HGYM_PROF_ROLLOUT = 10,  /* fused rollout step (policy + env step + previous finaliser); work = algorithmic HBM bytes */
    HGYM_PROF_COMM = 11,     /* hgym_comm_allreduce (the direct gradient exchange); work = bytes this rank moves over its links */
    HGYM_PROF_CLASSES = 12
};
int32_t hgym_prof_enable(int32_t on);  /* 1: start collecting (clears previous events), 0: stop */
int32_t hgym_prof_summary(int32_t cls, int64_t* launches, double* total_ms, double* work);
/* Kernel-internal phase clock for tuning the fused MLP kernels: while a caller-owned device buffer of `slots` int64 is set, thread 0
 * of every workgroup of every fused MLP launch (forward, update, rollout step) writes the 100 MHz wall clock at up to 8 phase boundaries
 * into dev[g*8 + slot], g = blockIdx.y * gridDim.x + blockIdx.x.  A launch asks for G groups and is not instrumented at all unless
 * 8 G <= slots; slots nobody stamps keep the caller's contents.  NULL: off.  Not capturable in a hipGraph.
 *   forward (hgym_policy_act, hgym_mlp_forward, each piece of hgym_critic_values): G = tiles x nets in the launch (+ tiles for the
 *     finaliser's grid row of hgym_policy_act_fin, which stamps nothing); group = tile x of net y; slots 0 start, 1 first input chunk
 *     staged, 2 first layer's products, 3 its epilogue, 4 layer 1, 5 layer 2, 6 head.  With an activation other than ELU(1) every net
 *     is a launch of its own: net i writes behind the i * tiles groups of the nets before it.
 *   update tile (hgym_ppo_grad, hgym_bc_grad): G = ceil(B / 64) x nets (hgym_bc_grad: the actor alone); slots 0-6 as above, 7 end of the dZ
 *     chain; per-net launches laid out as above.
 *   hgym_rollout_step: G = 3 x num_envs / 32 whatever the launch's grid rows.  Rows 0 and 1: the column's actor tile (0-6) and its
 *     non-actor workgroup -- a critic tile (0-6, 7 its end behind its side jobs) or, in the 64-row layout, a side-job workgroup (0 start,
 *     1 draws done, 2 rows ahead stored, 7 end; 3-6 untouched).  Row 2 is written by OTHER workgroups: group 2 * gridDim.x + x holds
 *     the env part of column x's actor workgroup (0 its start, 1 history stored, 2 joints, 3 per-env chain and rewards, 4 staged out, 5 end)
 *     and, where the launch carries the previous finaliser, slot 6 = start of workgroup x of the finaliser's grid row and (x = 0) slot 7 =
 *     the finaliser's end; the two writers' stamps are ordered within each writer only.
 *   hgym_rollout_eval_step is never instrumented. */
int32_t hgym_prof_phase_buffer(void* dev, int64_t slots);

#ifdef __cplusplus
}
#endif
#endif /* HGYM_H_ */
