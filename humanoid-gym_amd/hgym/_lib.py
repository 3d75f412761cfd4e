"""ctypes binding of include/hgym.h (libhgym_hip.so).

There is deliberately NO fallback: if the HIP library is missing or fails to load, importing this module
raises, and every product class built on it is unusable.  (The CPU oracle under /oracle is test
infrastructure and is never imported from here.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HGYM_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libhgym_hip.so"))

NUM_DOF = 12
NUM_BODIES = 13
NUM_REWARDS = 22
OBS_FRAME = 47
PRIV_FRAME = 73
MAX_LAYERS = 8
MAX_CUSTOM_REWARDS = 24
F32, BF16 = 0, 1
MIRROR_MAX_WIDTH = 2048     # HGYM_MIRROR_MAX_WIDTH
ACT_ELU, ACT_SELU, ACT_LEAKY_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4    # HGYM_ACT_*
STD_SCALAR, STD_LOG = 0, 1    # HGYM_STD_*: params[:A] hold sigma / log sigma (HgymNetConfig.std_param)

c_float_p = C.POINTER(C.c_float)
c_u8_p = C.POINTER(C.c_uint8)
c_i64_p = C.POINTER(C.c_int64)
c_f64_p = C.POINTER(C.c_double)


class EnvConfig(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32), ("frame_stack", C.c_int32), ("c_frame_stack", C.c_int32), ("decimation", C.c_int32),
        ("sim_dt", C.c_float), ("dt", C.c_float),
        ("max_episode_length", C.c_int32), ("resample_steps", C.c_int32), ("push_interval", C.c_int32),
        ("push_robots", C.c_int32), ("add_noise", C.c_int32), ("heading_command", C.c_int32), ("use_ref_actions", C.c_int32),
        ("clip_actions", C.c_float), ("clip_obs", C.c_float), ("action_scale", C.c_float),
        ("action_delay", C.c_float), ("action_noise", C.c_float), ("noise_level", C.c_float),
        ("obs_noise", C.c_float * OBS_FRAME),
        ("scale_lin_vel", C.c_float), ("scale_ang_vel", C.c_float), ("scale_dof_pos", C.c_float),
        ("scale_dof_vel", C.c_float), ("scale_quat", C.c_float),
        ("cmd_x_lo", C.c_float), ("cmd_x_span", C.c_float), ("cmd_y_lo", C.c_float), ("cmd_y_span", C.c_float),
        ("cmd_h_lo", C.c_float), ("cmd_h_span", C.c_float),
        ("dof_reset_lo", C.c_float), ("dof_reset_span", C.c_float),
        ("push_vel_lo", C.c_float), ("push_vel_span", C.c_float), ("push_ang_lo", C.c_float), ("push_ang_span", C.c_float),
        ("p_gains", C.c_float * NUM_DOF), ("d_gains", C.c_float * NUM_DOF), ("torque_limits", C.c_float * NUM_DOF),
        ("default_dof_pos", C.c_float * NUM_DOF), ("dof_lower", C.c_float * NUM_DOF), ("dof_upper", C.c_float * NUM_DOF),
        ("base_init_state", C.c_float * 13),
        ("base_body", C.c_int32), ("feet_bodies", C.c_int32 * 2), ("knee_bodies", C.c_int32 * 2),
        ("reward_scales", C.c_float * NUM_REWARDS), ("only_positive_rewards", C.c_int32),
        ("base_height_target", C.c_float), ("min_dist", C.c_float), ("max_dist", C.c_float),
        ("target_joint_pos_scale", C.c_float), ("target_feet_height", C.c_float), ("cycle_time", C.c_float),
        ("tracking_sigma", C.c_float), ("max_contact_force", C.c_float), ("episode_length_s", C.c_float),
        ("seed", C.c_uint64),
        # generic LeggedRobot options (all zero for XBot-L)
        ("custom_origins", C.c_int32), ("terrain_curriculum", C.c_int32), ("terrain_rows", C.c_int32), ("terrain_cols", C.c_int32),
        ("terrain_env_length", C.c_float), ("num_height_points", C.c_int32), ("height_rows", C.c_int32), ("height_cols", C.c_int32),
        ("terrain_border", C.c_float), ("terrain_hscale", C.c_float), ("terrain_vscale", C.c_float),
        ("cmd_yaw_lo", C.c_float), ("cmd_yaw_span", C.c_float),
        ("command_curriculum", C.c_int32), ("max_curriculum", C.c_float),
        # user-defined reward terms
        ("num_custom_rewards", C.c_int32), ("custom_reward_pos", C.c_int32 * MAX_CUSTOM_REWARDS),
    ]


class Strided(C.Structure):
    _fields_ = [("base", c_float_p), ("env_stride", C.c_int64), ("comp_stride", C.c_int64)]


class SimTensors(C.Structure):
    _fields_ = [("root", Strided), ("dof_pos", Strided), ("dof_vel", Strided), ("contact", Strided), ("rigid", Strided)]


ENV_STATE_FIELDS = [  # (name, components) in header order; all [C][N] fp32
    ("commands", 4), ("actions", 12), ("last_actions", 12), ("last_last_actions", 12), ("last_dof_vel", 12),
    ("last_root_vel", 6), ("torques", 12), ("feet_air_time", 2), ("last_contacts", 2), ("feet_height", 2),
    ("last_feet_z", 2), ("ref_dof_pos", 12), ("push_force", 3), ("push_torque", 3), ("episode_sums", NUM_REWARDS),
    ("base_lin_vel", 3), ("base_ang_vel", 3), ("projected_gravity", 3), ("base_euler", 3), ("friction", 1),
    ("body_mass", 1), ("env_origins", 3),
]


class EnvState(C.Structure):
    _fields_ = ([("episode_length", c_i64_p), ("counters", c_i64_p)] + [(n, c_float_p) for n, _ in ENV_STATE_FIELDS] +
                [("obs_ring", c_float_p), ("priv_ring", c_float_p), ("episode_acc", c_float_p),
                 ("terrain_levels", c_i64_p), ("terrain_types", c_i64_p), ("terrain_origins", c_float_p),
                 ("height_samples", C.POINTER(C.c_int16)), ("height_points", c_float_p), ("height_pose", c_float_p),
                 ("measured_heights", c_float_p), ("command_range_x", c_f64_p),
                 ("custom_rew", c_float_p), ("custom_sums", c_float_p), ("custom_acc", c_float_p)])


class EnvOut(C.Structure):
    _fields_ = [("obs", c_float_p), ("priv_obs", c_float_p), ("rew", c_float_p), ("reset", c_u8_p), ("time_out", c_u8_p),
                ("extras_time_outs", c_u8_p), ("extras_episode", c_float_p),
                ("t_values", c_float_p), ("t_rewards", c_float_p), ("t_dones", c_u8_p), ("t_step", c_i64_p),
                ("t_gamma", C.c_float), ("defer_finalize", C.c_int32), ("log_cur", c_float_p), ("log_stats", c_float_p),
                ("extras_custom", c_float_p), ("obs_ahead", c_float_p), ("priv_ahead", c_float_p), ("obs_older_ready", C.c_int32),
                ("l0_ahead", c_float_p), ("l0_ready", c_float_p), ("obs_bf16_ahead", C.c_void_p), ("ld_obs_bf16_ahead", C.c_int64),
                ("t_time_outs", c_u8_p)]


class EnvNoise(C.Structure):
    _fields_ = [("u_delay", c_float_p), ("z_act", c_float_p), ("u_cmd", c_float_p), ("u_dof", c_float_p),
                ("u_push", c_float_p), ("z_obs", c_float_p), ("u_xy", c_float_p), ("r_level", c_i64_p)]


class NetConfig(C.Structure):
    _fields_ = [("num_obs", C.c_int32), ("num_priv", C.c_int32), ("num_actions", C.c_int32),
                ("actor_layers", C.c_int32), ("critic_layers", C.c_int32),
                ("actor_dims", C.c_int32 * (MAX_LAYERS + 1)), ("critic_dims", C.c_int32 * (MAX_LAYERS + 1)),
                ("precision", C.c_int32), ("max_batch", C.c_int32),
                ("aux_layers", C.c_int32), ("aux_dims", C.c_int32 * (MAX_LAYERS + 1)), ("aux_target_offset", C.c_int32),
                ("activation", C.c_int32), ("act_alpha", C.c_float), ("act_scale", C.c_float),
                ("std_param", C.c_int32), ("fused_activation", C.c_int32)]


class PPOConfig(C.Structure):
    _fields_ = [("clip_param", C.c_float), ("value_loss_coef", C.c_float), ("entropy_coef", C.c_float),
                ("max_grad_norm", C.c_float), ("desired_kl", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
                ("lr_min", C.c_double), ("lr_max", C.c_double), ("adaptive_lr", C.c_int32), ("world_size", C.c_int32),
                ("aux_coef", C.c_float), ("grad_norm_ready", C.c_int32),
                ("value_loss_unclipped", C.c_int32)]

    # HgymPPOConfig.mirror_coef (float): appended behind value_loss_unclipped, in the four bytes that were the struct's tail padding (the two
    # doubles align it to 8) -- the size and every earlier offset are what they were, so `_fields_` still ends where its tests pin it and
    # the new member is reached at its offset.  A fresh PPOConfig() is zero-filled, padding included: off.
    @property
    def mirror_coef(self):
        return C.c_float.from_address(C.addressof(self) + MIRROR_COEF_OFFSET).value

    @mirror_coef.setter
    def mirror_coef(self, v):
        C.c_float.from_address(C.addressof(self) + MIRROR_COEF_OFFSET).value = v


MIRROR_COEF_OFFSET = PPOConfig.value_loss_unclipped.offset + 4
assert MIRROR_COEF_OFFSET + 4 <= C.sizeof(PPOConfig)


class Net(C.Structure):
    _fields_ = [("params", c_float_p), ("grads", c_float_p), ("adam_m", c_float_p), ("adam_v", c_float_p),
                ("opt_state", c_f64_p), ("workspace", C.c_void_p), ("norm", C.c_void_p)]


class Comm(C.Structure):
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("data", c_float_p * 8), ("flags", C.POINTER(C.c_uint32) * 8),
                ("count", C.c_int64), ("status", c_i64_p), ("wait_ticks", C.c_int64), ("aux", c_f64_p * 8)]


class Batch(C.Structure):
    _fields_ = [("obs", c_float_p), ("priv", c_float_p), ("actions", c_float_p), ("values", c_float_p),
                ("advantages", c_float_p), ("returns", c_float_p), ("logp", c_float_p), ("mu", c_float_p),
                ("sigma", c_float_p), ("idx", c_i64_p), ("B", C.c_int32),
                ("obs_bf16", C.c_void_p), ("priv_bf16", C.c_void_p), ("num_rows", C.c_int64),
                # the mirror loss (PPOConfig.mirror_coef > 0; a zero-filled tail is off)
                ("pair_idx", c_i64_p), ("mirror_act_src", C.POINTER(C.c_int32)), ("mirror_act_sign", c_float_p),
                ("mirror_target", c_float_p), ("mirror_sums", c_f64_p)]


BC_MSE, BC_HUBER = 0, 1    # HGYM_BC_*


class BCConfig(C.Structure):
    """HgymBCConfig: the loss of a behaviour-cloning minibatch (hgym_bc_grad)."""
    _fields_ = [("loss_type", C.c_int32), ("huber_delta", C.c_float)]


class VFConfig(C.Structure):
    """HgymVFConfig: the value loss of a critic-only minibatch (hgym_vf_grad, hgym_bc_vf_grad)."""
    _fields_ = [("clip_param", C.c_float), ("value_coef", C.c_float), ("unclipped", C.c_int32), ("keep_others", C.c_int32)]


class ObsShadow(C.Structure):
    """HgymObsShadow: where a policy launch leaves the bf16 of the observation rows it reads (row-major, ld in elements)."""
    _fields_ = [("obs", C.c_void_p), ("ld_obs", C.c_int64), ("priv", C.c_void_p), ("ld_priv", C.c_int64)]


RND_MAX_OUTPUTS = 64     # HGYM_RND_MAX_OUTPUTS
RND_CONSTANT, RND_STEP, RND_LINEAR = 0, 1, 2    # HGYM_RND_*: HgymRndConfig.schedule


class RndConfig(C.Structure):
    """HgymRndConfig: the discount, the weight schedule and the normalisation switch of hgym_rnd_rewards."""
    _fields_ = [("gamma", C.c_double), ("weight", C.c_double), ("final_value", C.c_double), ("initial_step", C.c_int64),
                ("final_step", C.c_int64), ("schedule", C.c_int32), ("normalize", C.c_int32)]


SLOT_PERTURB = 128       # hgym_common.hpp slot map: 128 .. 128 + ceil(width / 4) - 1 = the normals of one row of hgym_perturb_rows


class Smooth(C.Structure):
    """HgymSmooth: the coefficients, the successor map, the perturbation and the caller-owned scratch of hgym_ppo_grad_smooth."""
    _fields_ = [("temporal_coef", C.c_float), ("spatial_coef", C.c_float), ("next_idx", c_i64_p), ("next_weight", c_float_p),
                ("noise_std", c_float_p), ("seed", C.c_uint64), ("target_next", c_float_p), ("target_near", c_float_p),
                ("rows", c_float_p), ("sums", c_f64_p)]


GUIDE_CONSTANT, GUIDE_STEP, GUIDE_LINEAR = 0, 1, 2    # HGYM_GUIDE_*: HgymGuideSchedule.mode


class GuideSchedule(C.Structure):
    """HgymGuideSchedule: the coefficient of the guidance term as a function of the update count (hgym_guide_schedule)."""
    _fields_ = [("coef", C.c_double), ("final_value", C.c_double), ("initial_step", C.c_int64), ("final_step", C.c_int64),
                ("mode", C.c_int32), ("reserved", C.c_int32)]


class Guide(C.Structure):
    """HgymGuide: the teacher's mean column, the device-resident coefficient and the two sums of hgym_ppo_grad_guide."""
    _fields_ = [("teacher_mu", c_float_p), ("coef", c_float_p), ("sums", c_f64_p)]


STRUCTS = dict(HgymEnvConfig=EnvConfig, HgymStrided=Strided, HgymSimTensors=SimTensors, HgymEnvState=EnvState,
               HgymEnvOut=EnvOut, HgymEnvNoise=EnvNoise, HgymNetConfig=NetConfig, HgymPPOConfig=PPOConfig,
               HgymNet=Net, HgymBatch=Batch, HgymObsShadow=ObsShadow, HgymComm=Comm, HgymBCConfig=BCConfig, HgymRndConfig=RndConfig,
               HgymSmooth=Smooth, HgymGuideSchedule=GuideSchedule, HgymGuide=Guide, HgymVFConfig=VFConfig)

# every symbol include/hgym.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "hgym_comm_alloc": (C.c_int32, [C.c_int64, C.POINTER(C.c_void_p)]),
    "hgym_comm_free": (C.c_int32, [C.c_void_p]),
    "hgym_comm_ipc_export": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "hgym_comm_ipc_open": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "hgym_comm_ipc_close": (C.c_int32, [C.c_void_p]),
    "hgym_comm_allreduce": (C.c_int32, [_P(Comm), C.c_uint32, C.c_void_p]),
    "hgym_comm_status": (C.c_int32, [_P(Comm), c_i64_p, C.c_void_p]),
    "hgym_comm_sum64": (C.c_int32, [_P(Comm), c_f64_p, C.c_int32, C.c_void_p]),
    "hgym_version": (C.c_int32, []),
    "hgym_last_error": (C.c_char_p, []),
    "hgym_device_cus": (C.c_int32, []),
    "hgym_sizeof": (C.c_int64, [C.c_char_p]),
    "hgym_env_config_default": (C.c_int32, [_P(EnvConfig), C.c_int32]),
    "hgym_env_prime": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), C.c_void_p]),
    "hgym_env_reset_all": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), C.c_void_p]),
    "hgym_env_reset_idx": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), c_i64_p, C.c_int32, c_u8_p,
                                       c_i64_p, C.c_void_p]),
    "hgym_pre_physics": (C.c_int32, [_P(EnvConfig), _P(EnvState), c_float_p, _P(EnvNoise), C.c_void_p]),
    "hgym_pd_torques": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), C.c_void_p]),
    "hgym_synth_physics": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), C.c_void_p]),
    "hgym_post_physics": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), C.c_void_p]),
    "hgym_env_step_synth": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), c_float_p, C.c_void_p]),
    "hgym_env_finalize": (C.c_int32, [_P(EnvConfig), _P(EnvState), _P(EnvOut), C.c_void_p]),
    "hgym_env_step_begin": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), c_float_p, C.c_void_p]),
    "hgym_env_step_end": (C.c_int32, [_P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvNoise), C.c_void_p]),
    "hgym_measure_heights": (C.c_int32, [_P(EnvConfig), _P(EnvState), C.c_void_p]),
    "hgym_store_step": (C.c_int32, [C.c_int32, c_float_p, c_float_p, c_u8_p, c_u8_p, C.c_float, c_float_p, c_u8_p, C.c_void_p]),
    "hgym_randperm": (C.c_int32, [C.c_int64, C.c_uint64, C.c_uint64, c_i64_p, C.c_void_p]),
    "hgym_randperm_dev": (C.c_int32, [C.c_int64, C.c_uint64, c_i64_p, c_i64_p, C.c_void_p]),
    "hgym_gae": (C.c_int32, [C.c_int32, C.c_int32, c_float_p, c_float_p, c_u8_p, c_float_p, C.c_float, C.c_float,
                             c_float_p, c_float_p, c_f64_p, C.c_void_p]),
    "hgym_adv_normalize": (C.c_int32, [C.c_int64, c_float_p, c_f64_p, C.c_void_p]),
    "hgym_adv_normalize_minibatches": (C.c_int32, [C.c_int32, C.c_int64, c_i64_p, c_float_p, c_float_p, C.c_int64, c_f64_p, C.c_void_p]),
    "hgym_value_denormalize": (C.c_int32, [C.c_int64, c_float_p, c_float_p, c_f64_p, C.c_float, C.c_void_p]),
    "hgym_value_norm_merge": (C.c_int32, [C.c_int64, c_float_p, c_f64_p, c_f64_p, C.c_void_p]),
    "hgym_value_normalize": (C.c_int32, [C.c_int64, c_float_p, c_f64_p, C.c_float, C.c_void_p]),
    "hgym_rnd_block_init": (C.c_int32, [C.c_int32, c_f64_p, C.c_void_p]),
    "hgym_rnd_rewards": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, _P(RndConfig), c_f64_p,
                                     C.c_void_p]),
    "hgym_gae_bootstrap": (C.c_int32, [C.c_int32, C.c_int32, c_float_p, c_float_p, c_u8_p, c_u8_p, c_float_p, C.c_float, C.c_float,
                                       c_float_p, c_float_p, c_f64_p, C.c_void_p]),
    "hgym_mirror_rows": (C.c_int32, [C.c_int64, C.c_int32, C.POINTER(C.c_int32), c_float_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_int32, C.c_void_p]),
    "hgym_critic_values": (C.c_int32, [_P(NetConfig), _P(Net), C.c_int64, c_float_p, c_float_p, _P(ObsShadow), C.c_void_p]),
    "hgym_net_param_count": (C.c_int64, [_P(NetConfig)]),
    "hgym_net_workspace_bytes": (C.c_int64, [_P(NetConfig)]),
    "hgym_net_sigma_offset": (C.c_int64, [_P(NetConfig)]),
    "hgym_net_sync_shadow": (C.c_int32, [_P(NetConfig), _P(Net), C.c_void_p]),
    "hgym_net_norm_layout": (C.c_int32, [_P(NetConfig), c_i64_p]),
    "hgym_net_norm_init": (C.c_int32, [_P(NetConfig), _P(Net), C.c_float, C.c_int64, C.c_void_p]),
    "hgym_net_norm_accumulate": (C.c_int32, [_P(NetConfig), _P(Net), c_float_p, c_float_p, C.c_int64, C.c_void_p]),
    "hgym_net_norm_merge": (C.c_int32, [_P(NetConfig), _P(Net), C.c_void_p]),
    "hgym_net_norm_unfold_grad": (C.c_int32, [_P(NetConfig), _P(Net), C.c_void_p]),
    "hgym_mlp_forward": (C.c_int32, [_P(NetConfig), _P(Net), C.c_int32, C.c_int32, c_float_p, C.c_int64, c_float_p, C.c_void_p]),
    "hgym_net_shadow_ld": (C.c_int64, [_P(NetConfig), C.c_int32]),
    "hgym_policy_act": (C.c_int32, [_P(NetConfig), _P(Net), C.c_int32, c_float_p, c_float_p, c_float_p, C.c_uint64, c_i64_p,
                                    c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, _P(ObsShadow), C.c_void_p]),
    "hgym_policy_act_fin": (C.c_int32, [_P(NetConfig), _P(Net), C.c_int32, c_float_p, c_float_p, c_float_p, C.c_uint64, c_i64_p,
                                    c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, _P(EnvConfig), _P(EnvState), _P(EnvOut),
                                    _P(ObsShadow), C.c_void_p]),
    "hgym_rollout_begin": (C.c_int32, [_P(EnvState), c_i64_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "hgym_rollout_step": (C.c_int32, [_P(NetConfig), _P(Net), _P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvOut), c_float_p,
                                      c_float_p, C.c_uint64, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_void_p, C.c_int32,
                                      _P(ObsShadow), C.c_void_p]),
    "hgym_rollout_step_z": (C.c_int32, [_P(NetConfig), _P(Net), _P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvOut), c_float_p,
                                        c_float_p, C.c_uint64, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_void_p, C.c_int32,
                                        _P(ObsShadow), C.c_void_p, c_float_p]),
    "hgym_policy_noise_table": (C.c_int32, [C.c_int32, C.c_int64, C.c_int32, c_float_p, C.c_int64, c_float_p, c_float_p, C.c_uint64, c_i64_p,
                                            c_float_p, C.c_void_p]),
    "hgym_rollout_end": (C.c_int32, [_P(EnvConfig), _P(EnvState), _P(EnvOut), C.c_void_p, C.c_int32, C.c_void_p]),
    "hgym_rollout_eval_step": (C.c_int32, [_P(NetConfig), _P(Net), _P(EnvConfig), _P(SimTensors), _P(EnvState), _P(EnvOut), _P(EnvOut), c_float_p,
                                           c_float_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "hgym_eval_reset": (C.c_int32, [C.c_int32, c_f64_p, C.c_void_p]),
    "hgym_eval_accumulate": (C.c_int32, [C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_u8_p, c_u8_p, c_f64_p, C.c_void_p]),
    "hgym_ppo_diag_reset": (C.c_int32, [C.c_int64, c_f64_p, C.c_void_p]),
    "hgym_ppo_diag_reduce": (C.c_int32, [C.c_int64] + [c_float_p] * 10 + [C.c_float, C.c_int64, C.c_int64, C.c_int32, c_f64_p, C.c_void_p]),
    "hgym_ppo_diagnostics": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), C.c_int64, c_float_p, c_f64_p, C.c_void_p]),
    "hgym_ppo_grad": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), C.c_void_p]),
    "hgym_ppo_grad_part": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), C.c_int32, C.c_void_p]),
    "hgym_bc_grad": (C.c_int32, [_P(NetConfig), _P(BCConfig), _P(Net), _P(Batch), c_float_p, c_f64_p, C.c_void_p]),
    "hgym_vf_grad": (C.c_int32, [_P(NetConfig), _P(VFConfig), _P(Net), _P(Batch), c_f64_p, C.c_void_p]),
    "hgym_bc_vf_grad": (C.c_int32, [_P(NetConfig), _P(BCConfig), _P(VFConfig), _P(Net), _P(Batch), c_float_p, c_f64_p, c_f64_p, C.c_void_p]),
    "hgym_smooth_pairs": (C.c_int32, [C.c_int64, C.c_int64, c_i64_p, c_u8_p, c_i64_p, c_float_p, C.c_void_p]),
    "hgym_perturb_rows": (C.c_int32, [C.c_int64, C.c_int32, c_float_p, C.c_int64, c_i64_p, c_float_p, C.c_uint64, c_f64_p, c_float_p, C.c_int64,
                                      C.c_void_p]),
    "hgym_ppo_grad_smooth": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), _P(Smooth), C.c_void_p]),
    "hgym_ppo_grad_smooth_mirror": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), _P(Smooth), c_float_p, C.c_int64, C.c_void_p]),
    "hgym_guide_schedule": (C.c_int32, [_P(GuideSchedule), c_i64_p, c_float_p, C.c_void_p]),
    "hgym_ppo_grad_guide": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), _P(Batch), _P(Guide), C.c_void_p]),
    "hgym_net_param_offset": (C.c_int64, [_P(NetConfig), C.c_int32]),
    "hgym_ppo_apply": (C.c_int32, [_P(NetConfig), _P(PPOConfig), _P(Net), C.c_void_p]),
    "hgym_prof_enable": (C.c_int32, [C.c_int32]),
    "hgym_prof_phase_buffer": (C.c_int32, [C.c_void_p, C.c_int64]),
    "hgym_prof_summary": (C.c_int32, [C.c_int32, _P(C.c_int64), _P(C.c_double), _P(C.c_double)]),
}
PROF_GEMM, PROF_ENV_STEP, PROF_GAE, PROF_LOSS, PROF_MLP_FWD, PROF_MLP_BWD, PROF_DW, PROF_REDUCE, PROF_APPLY, PROF_POLICY, PROF_ROLLOUT, PROF_COMM = range(12)
NOISE_MAX_STEPS = 128     # HGYM_NOISE_MAX_STEPS: the longest table hgym_policy_noise_table fills
SLOT_POLICY = 64          # hgym_common.hpp slot map: 64 .. 66 = the 12 policy-sampling normals of one env and step
ROLLOUT_SCRATCH_HEADER_BYTES = 512
ROLLOUT_DRAW_BYTES_PER_ENV = 1000


def rollout_scratch_bytes(num_envs):
    """HGYM_ROLLOUT_SCRATCH_BYTES(num_envs) of include/hgym.h."""
    return ROLLOUT_SCRATCH_HEADER_BYTES + ROLLOUT_DRAW_BYTES_PER_ENV * int(num_envs)

# HgymEnvOut.log_stats (include/hgym.h: HGYM_LOG_*)
LOG_STATS = 256
LOG_TERMS, LOG_STEPS, LOG_CLEAR, LOG_RING_HEAD, LOG_RING_FILL = 0, 22, 23, 24, 25
LOG_RING, LOG_RETURNS, LOG_LENGTHS = 100, 32, 132
# HgymEnvState.counters (HGYM_CNT_*)
CNT_STEP, CNT_RESETS, CNT_RING, CNT_RESET_CALL = range(4)
# hgym_net_norm_layout (HGYM_NORM_*): slots of the layout array; +k: 0 actor / obs, 1 critic / priv (BIAS: + net)
NORM_LAYOUT = 24
(NORM_BYTES, NORM_HEADER, NORM_MEAN, NORM_VAR, NORM_MEAN_F, NORM_SCALE_F, NORM_BIAS, NORM_SUMS, NORM_SUMS_DOUBLES, NORM_PARTIALS, NORM_WGS,
 NORM_ROWS_PER_WG) = (0, 1, 2, 4, 6, 8, 10, 13, 14, 15, 17, 19)
NORM_HEADER_DOUBLES = 8     # eps, until, count (actor), count (critic), unused
# HgymNet.opt_state (HGYM_OPT_*)
OPT_STATE = 16
(OPT_LR, OPT_STEP, OPT_KL_SUM, OPT_SURROGATE_SUM, OPT_VALUE_SUM, OPT_ENTROPY_SUM, OPT_GRAD_NORM, OPT_MINIBATCHES, OPT_KL_LAST,
 OPT_GRAD_SQNORM, OPT_AUX_SUM, OPT_STEP_SIZE, OPT_SQRT_BC2, OPT_PROLOGUE_STEP, OPT_BETA1_POW, OPT_BETA2_POW) = range(16)


def prof_summary(cls):
    n, ms, work = C.c_int64(), C.c_double(), C.c_double()
    rc = lib.hgym_prof_summary(cls, C.byref(n), C.byref(ms), C.byref(work))
    if rc != 0:
        raise HgymError("hgym_prof_summary failed: %s" % lib.hgym_last_error().decode())
    return n.value, ms.value, work.value


class HgymError(RuntimeError):
    pass


def _load(path):
    if not os.path.exists(path):
        raise ImportError(
            "libhgym_hip.so not found at %s -- build it with `python humanoid-gym_amd/build.py` "
            "(there is no CPU fallback for the hot path)" % path)
    lib = C.CDLL(path)
    missing = []
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise ImportError("libhgym_hip.so lacks symbols declared in include/hgym.h: %s" % ", ".join(missing))
    return lib


lib = _load(LIB_PATH)


def check(rc, what=""):
    if rc != 0:
        raise HgymError("%s failed (%d): %s" % (what or "hgym call", rc, lib.hgym_last_error().decode()))


def fptr(t):
    """float* of a torch tensor (or None)."""
    return None if t is None else C.cast(t.data_ptr(), c_float_p)


def u8ptr(t):
    return None if t is None else C.cast(t.data_ptr(), c_u8_p)


def i64ptr(t):
    return None if t is None else C.cast(t.data_ptr(), c_i64_p)


def f64ptr(t):
    return None if t is None else C.cast(t.data_ptr(), c_f64_p)


# the evaluation accumulator's block (include/hgym.h: HGYM_EVAL_*)
EVAL_SUMS, EVAL_ENVS_PER_PARTIAL = 32, 256
EVAL_STEPS, EVAL_ENV_STEPS, EVAL_LIN_ERR, EVAL_ANG_ERR, EVAL_REWARD, EVAL_EPISODES, EVAL_TIMEOUTS, EVAL_RETURN, EVAL_LENGTH = range(9)
EVAL_TICKET, EVAL_TERMS = 9, 10


def eval_block_doubles(n):
    """HGYM_EVAL_BLOCK_DOUBLES(n) of include/hgym.h."""
    n = int(n)
    return EVAL_SUMS * (1 + (n + EVAL_ENVS_PER_PARTIAL - 1) // EVAL_ENVS_PER_PARTIAL) + 24 * n


def eval_block(n, device):
    """The accumulator block of hgym_eval_reset / hgym_eval_accumulate for n envs, zero-filled."""
    import torch
    return torch.zeros(eval_block_doubles(n), dtype=torch.float64, device=device)


def gae_stats(n, device):
    """The `stats` buffer of hgym_gae / hgym_gae_bootstrap for n envs: HGYM_GAE_STATS_DOUBLES(n) zero-filled doubles (include/hgym.h)."""
    import torch
    return torch.zeros(4 + 2 * ((int(n) + 15) // 16), dtype=torch.float64, device=device)


ADV_MB_CHUNK = 1024     # entries of a segment whose partial sums one workgroup of hgym_adv_normalize_minibatches forms


def adv_mb_scratch_doubles(segments, seg_len):
    """HGYM_ADV_MB_SCRATCH_DOUBLES(segments, seg_len) of include/hgym.h."""
    return int(segments) * (3 + 2 * ((int(seg_len) + ADV_MB_CHUNK - 1) // ADV_MB_CHUNK))


def adv_mb_scratch(segments, seg_len, device):
    """The `scratch` buffer of hgym_adv_normalize_minibatches, zero-filled."""
    import torch
    return torch.zeros(adv_mb_scratch_doubles(segments, seg_len), dtype=torch.float64, device=device)


# value-target normalisation (include/hgym.h: HGYM_VALUE_NORM_*)
VALUE_NORM_BLOCK_DOUBLES, VALUE_NORM_CHUNK, VALUE_NORM_MAX_BLOCKS = 3, 1024, 1024
VALUE_NORM_COUNT, VALUE_NORM_MEAN, VALUE_NORM_VAR = range(3)      # the block's slots
VALUE_NORM_BATCH, VALUE_NORM_TICKET, VALUE_NORM_PARTIALS = 0, 3, 4      # the scratch's


def value_norm_scratch_doubles(n):
    """HGYM_VALUE_NORM_SCRATCH_DOUBLES(n) of include/hgym.h."""
    return VALUE_NORM_PARTIALS + 2 * ((int(n) + VALUE_NORM_CHUNK - 1) // VALUE_NORM_CHUNK)


def value_norm_scratch(n, device):
    """The `scratch` buffer of hgym_value_norm_merge for n values, zero-filled."""
    import torch
    return torch.zeros(value_norm_scratch_doubles(n), dtype=torch.float64, device=device)


def value_norm_block(device):
    """The `block` of the hgym_value_* calls in its initial state: count 0, mean 0, var 1."""
    import torch
    return torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=device)


# the diagnostics pass's block (include/hgym.h: HGYM_DIAG_*)
DIAG_SUMS, DIAG_ROWS_PER_PARTIAL = 16, 256
(DIAG_COUNT, DIAG_KL, DIAG_APPROX_KL, DIAG_RATIO, DIAG_CLIPPED, DIAG_RATIO_MAX, DIAG_RATIO_MIN, DIAG_SURROGATE, DIAG_RET, DIAG_RET_SQ,
 DIAG_ERR_OLD, DIAG_ERR_OLD_SQ, DIAG_ERR_NEW, DIAG_ERR_NEW_SQ, DIAG_VALUE_CLIPPED, DIAG_ENTROPY) = range(16)


def diag_block_doubles(total_rows):
    """HGYM_DIAG_BLOCK_DOUBLES(total_rows) of include/hgym.h."""
    return DIAG_SUMS * (1 + (int(total_rows) + DIAG_ROWS_PER_PARTIAL - 1) // DIAG_ROWS_PER_PARTIAL)


def diag_block(total_rows, device):
    """The block of hgym_ppo_diag_reset / hgym_ppo_diag_reduce / hgym_ppo_diagnostics for total_rows rows, zero-filled."""
    import torch
    return torch.zeros(diag_block_doubles(total_rows), dtype=torch.float64, device=device)


# the RND reward pass's block (include/hgym.h: HGYM_RND_*)
RND_HEADER, RND_ROWS_PER_WG, RND_ENVS_PER_PARTIAL, RND_APPLY_WGS = 16, 64, 64, 1024
(RND_MEAN, RND_VAR, RND_COUNT, RND_COUNTER, RND_SUM_INTRINSIC, RND_SUM_REWARDS, RND_WEIGHT_LAST, RND_STD, RND_ROWS, RND_TICKET_SCAN,
 RND_TICKET_APPLY) = range(11)


def rnd_block_doubles(n):
    """HGYM_RND_BLOCK_DOUBLES(n) of include/hgym.h."""
    n = int(n)
    return RND_HEADER + n + 2 * ((n + RND_ENVS_PER_PARTIAL - 1) // RND_ENVS_PER_PARTIAL) + 2 * RND_APPLY_WGS


def rnd_block(n, device):
    """The state block of hgym_rnd_rewards for n envs on a GPU, written by hgym_rnd_block_init on that device's current stream."""
    import torch
    b = torch.empty(rnd_block_doubles(n), dtype=torch.float64, device=device)
    assert b.is_cuda, "the block lives on the device (hgym_rnd_block_init writes it)"
    with torch.cuda.device(b.device):
        check(lib.hgym_rnd_block_init(int(n), f64ptr(b), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_rnd_block_init")
    return b
