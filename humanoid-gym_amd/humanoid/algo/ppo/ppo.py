"""PPO with the reference's interface (algo/ppo/ppo.py:38-184) on the MI355X hot path.

act() = one hgym_policy_act call whose outputs land directly in the rollout-storage slot; process_env_step() =
hgym_store_step (time-out bootstrap) ; compute_returns() = wavefront-scan GAE ; update() = for every minibatch
hgym_ppo_grad (gather + forward + KL + loss + hand-written backward, all on the device, no host sync) ->
[when torch.distributed is initialised: one RCCL all-reduce of [flat gradient | minibatch KL]] -> hgym_ppo_apply (adaptive-KL
learning rate, grad-norm clip, Adam, operand-shadow refresh).  The host reads the loss sums back once per update.
"""
import ctypes as C
import math
import os

import torch
import torch.nn as nn  # noqa: F401  (kept importable like the reference module)

from .actor_critic import ActorCritic
from .log_block import LogBlock
from .mirror_loss import MirrorLoss
from .normalizer import ValueNormalizer
from .rollout_storage import RolloutStorage
from . import critic_warmup as warmup_module
from . import dist_utils
from . import exploration_noise as noise_module
from . import guidance as guide_module
from . import rnd as rnd_module
from . import smoothness as smooth_module


def _struct_bytes(s):      # a ctypes structure's contents, hashable
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


class _DeviceAdam:
    """What `alg.optimizer` exposes to OnPolicyRunner.save/load: torch.optim.Adam-shaped state dicts backed by the
    flat exp_avg / exp_avg_sq vectors the HIP Adam kernel updates."""

    # the hyper-parameters the HIP Adam kernel runs with (hgym.make_ppo_config); ONE definition for param_groups and for the
    # runner's background checkpoint writer, which must not read the learning rate from the device (a host sync)
    HYPER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False)

    def __init__(self, ppo):
        self._ppo = ppo

    @property
    def param_groups(self):
        return [dict(lr=self._ppo.learning_rate, **self.HYPER)]

    def state_dict(self):
        net = self._ppo.net
        state = {}
        if net is not None:
            step = float(net.opt_state[self._ppo._hgym._lib.OPT_STEP])
            base = net.params.data_ptr()
            for i, (name, v) in enumerate(net.views.items()):
                o = (v.data_ptr() - base) // 4
                state[i] = dict(step=torch.tensor(step), exp_avg=net.adam_m[o:o + v.numel()].view_as(v).clone(),
                                exp_avg_sq=net.adam_v[o:o + v.numel()].view_as(v).clone())
        n = len(state)
        return dict(state=state, param_groups=[dict(self.param_groups[0], params=list(range(n)))])

    def load_state_dict(self, sd):
        net = self._ppo.net
        base = net.params.data_ptr()
        warm = getattr(self._ppo, "_warmup", None)
        if warm is not None:      # critic-only updates remain: the actor's moments must be zero (refused before anything is changed)
            warmup_module.check_moments(warm.remaining, [(name, sd["state"][i]["exp_avg"], sd["state"][i]["exp_avg_sq"])
                                                         for i, name in enumerate(net.views) if i in sd["state"]])
        for i, (name, v) in enumerate(net.views.items()):
            if i in sd["state"]:
                o = (v.data_ptr() - base) // 4
                net.adam_m[o:o + v.numel()].copy_(sd["state"][i]["exp_avg"].flatten())
                net.adam_v[o:o + v.numel()].copy_(sd["state"][i]["exp_avg_sq"].flatten())
                net.opt_state[self._ppo._hgym._lib.OPT_STEP] = float(sd["state"][i]["step"])
        if sd.get("param_groups"):
            self._ppo.learning_rate = sd["param_groups"][0]["lr"]

    def zero_grad(self):
        if self._ppo.net is not None:
            self._ppo.net.grads.zero_()


class PPO:
    actor_critic: ActorCritic
    # minibatch permutation: "device" = hgym_randperm (keyed bijection, one launch, reproducible from the seed);
    # "torch" = torch.randperm from torch's global generator, as the reference draws it (a device sort: 125 us per iteration)
    permutation = "device"
    # compute precision of the dense layers: "bf16" (MFMA fast path, BASELINE config) or "f32" (parity mode)
    precision = os.environ.get("HGYM_PRECISION", "bf16")
    # left-right symmetry augmentation: None, or a humanoid.utils.symmetry.MirrorSpec -- the update then also trains on the mirrored
    # transition of every stored row (RolloutStorage.enable_mirror / mirror), minibatches twice as large, as many Adam steps.  Read once,
    # in init_storage.  The adaptive learning-rate rule's KL is the fused loss's mean over the WHOLE minibatch, mirrored rows included
    # (rsl_rl averages it over the original rows only): it also sees the policy's asymmetry.  DESIGN.md section 21.
    symmetry = None
    # the mirror loss, the other half of rsl_rl's symmetry_cfg (use_mirror_loss / mirror_loss_coeff): mirror_loss_coef * mse(mu(s), M_a mu(M s))
    # added to the PPO loss, the target under the current parameters and detached (HgymPPOConfig.mirror_coef).  Needs `symmetry` (its
    # tables; ValueError otherwise).  symmetry_augmentation = False keeps the mirrored observations (the loss's partner rows) but trains on
    # the T N original rows only: minibatches of today's size, one more actor forward per minibatch; in that form it combines with
    # PPO.smoothness.  With the coefficient 0 it is the same as symmetry off.  Both read once, in init_storage.  `last_mirror_loss`: the mean MSE per minibatch of the last update.
    mirror_loss_coef = 0.0
    symmetry_augmentation = True
    # how the advantages are standardised: "batch" -- the reference's way, once over the whole T N batch at the end of compute_returns (the
    # all-reduced statistics on several ranks); "minibatch" -- rsl_rl's normalize_advantage_per_mini_batch: compute_returns leaves the raw
    # advantages, update() standardises every minibatch by its own mean and unbiased deviation (one segmented pass per update into
    # storage.advantages_mb, which the batch descriptor then names; nothing crosses ranks); "none" -- the raw advantages are used.  With
    # symmetry augmentation a minibatch's statistics are over its drawn rows, originals and mirrors alike (rsl_rl normalises before it
    # augments).  Read once, in init_storage.  DESIGN.md section 24.
    advantage_normalization = "batch"
    ADVANTAGE_NORMALIZATIONS = ("batch", "minibatch", "none")
    # Random Network Distillation (rsl_rl's rnd_cfg): None, or a humanoid.algo.ppo.rnd.RandomNetworkDistillation -- compute_returns then
    # adds an intrinsic exploration reward to the stored rewards ahead of GAE (one pass over the stored rows behind the rollout:
    # hgym_rnd_rewards), and update() follows every minibatch's Adam step with one step of the predictor on the same rows.  One rank, no
    # symmetry augmentation, not with Distillation (ValueError from init_storage).  Read once, in init_storage.  DESIGN.md section 27.
    rnd = None
    # the smoothness regulariser on the policy's mean, after CAPS: None, or a dict {temporal_coef, spatial_coef, noise_std, noise_scale, seed}
    # (humanoid.algo.ppo.smoothness.parse_config) -- update() then calls hgym_ppo_grad_smooth in place of hgym_ppo_grad: lamT pulls mu(s_t)
    # towards mu(s_t+1) over rows whose episode went on, lamS pulls mu(s) towards mu(s + noise_std z), both targets detached.  One rank, no
    # symmetry augmentation, not with Distillation (ValueError from init_storage).  Beside the mirror loss without augmentation
    # (mirror_loss_coef > 0, symmetry_augmentation = False) update() calls hgym_ppo_grad_smooth_mirror, one actor head for all three terms; the
    # spatial term's noise_std must then be invariant under the observation mirror table (ValueError naming the column).  Read once, in
    # init_storage.  `last_smoothness`: {temporal, spatial, valid_fraction} of the last update.  DESIGN.md sections 28 and 32.
    smoothness = None
    # value targets standardised by running statistics (rl_games' normalize_value, the return half of SB3's VecNormalize): the critic lives
    # in normalised units.  Per iteration: the critic's outputs are denormalised as they are stored (one launch behind the policy launch,
    # or behind deferred_values()), GAE and the advantages run on raw values, then compute_returns merges the T N raw returns into the
    # running (count, mean, var) -- ahead of the update, so the targets are normalised by statistics that already include them, as in
    # rl_games -- and puts `returns` and the old `values` into the critic's units.  No update kernel changes: the value clip range is
    # clip_param in normalised units.  ActorCritic.evaluate() keeps returning what the critic outputs (normalised); `value_normalizer`
    # (mean, var, std, count, forward, inverse) is the host's view.  A one-launch rollout takes the deferred critic.  One rank, not with
    # Distillation (ValueError from init_storage).  Both read once, in init_storage.  DESIGN.md section 31.
    value_normalization = False
    value_normalization_eps = 1e-2
    value_normalizer = None      # the option's object once init_storage has built it; here, so that a PPO made without __init__ has the handle too
    # guidance by a frozen teacher (kickstarting): None, or a dict {teacher, coef, coef_schedule, teacher_hidden_dims, teacher_activation,
    # teacher_max_batch} (humanoid.algo.ppo.guidance.parse_config) -- compute_returns then ends with the teacher's pass over the T N stored
    # observation rows (storage.teacher_mu), update() starts with hgym_guide_schedule (the coefficient of this update, formed and kept on
    # the device) and calls hgym_ppo_grad_guide in place of hgym_ppo_grad: coef / (B A) sum (mu - t)^2 joins the loss, t detached.  When a
    # schedule that ends at 0 has run out the update is the plain one again (one re-capture).  One rank, no symmetry in either form, not
    # with PPO.smoothness, not with Distillation (ValueError from init_storage).  Read once, in init_storage.  `last_guidance`: {loss, coef}
    # of the last update.  DESIGN.md section 33.
    guidance = None
    # critic-only warm-up: the first n updates of a run move the value function alone -- every minibatch step is hgym_vf_grad followed by
    # hgym_ppo_apply with the learning-rate rule off; the actor, sigma and the learning rate keep their bits (zero gradient on zero Adam
    # moments), and the actor-side options (mirror loss, smoothness, guidance and its schedule count) are not invoked.  For a checkpoint
    # without a usable critic: a plain distillation run, an older policy, a changed reward.  compute_returns, value normalisation, both
    # advantage modes and symmetry augmentation go on unchanged.  The count of updates done is host state: part of update_graph_key() (one
    # re-capture at the switch) and of a checkpoint.  One rank; an optimiser state with non-zero actor moments is refused while updates
    # remain (ValueError).  0: off.  Read once, in init_storage.  DESIGN.md section 34.
    critic_warmup_updates = 0
    # temporally correlated exploration noise: None, or a dict {"kind": "ar1", "rho": r} / {"kind": "colored", "beta": b}
    # (humanoid.algo.ppo.exploration_noise.parse_config) -- the normals of a rollout are a filtered sequence per (env, action) instead of
    # fresh white draws at every step: one launch at the head of every rollout fills a (T, N, A) table from the very draws the policy
    # launches would have made (hgym_policy_noise_table), and every policy launch reads its row in place of its own draw (act(): `z`; the
    # one-launch rollout: hgym_rollout_step_z).  Each x_t stays N(0, 1), so logp, sigma, the ratio and the update are what they were: PPO
    # treats the steps as independent.  The sequence does not restart at episode resets.  rho = 0 / beta = 0: the reference's noise, bit
    # for bit.  Combines with every other option, with Distillation and with several ranks (no test runs it on more than one rank); at most 128 steps per rollout (ValueError from
    # init_storage).  Read once, in init_storage.  DESIGN.md section 35.
    exploration_noise = None

    def __init__(self, actor_critic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True,
                 schedule="fixed", desired_kl=0.01, device="cpu", denoise_coef=0.0):
        if not (str(device).startswith("cuda") and torch.cuda.is_available()):
            raise RuntimeError("PPO runs on the MI355X hot path only (device=%r); there is no CPU training path" % (device,))
        self.device = device
        self.desired_kl, self.schedule = desired_kl, schedule
        self._lr0 = learning_rate
        self.actor_critic = actor_critic
        self.actor_critic.to(self.device)
        self.storage = None
        self.net = None
        self.optimizer = _DeviceAdam(self)
        self.transition = RolloutStorage.Transition()
        self.clip_param = clip_param
        self.num_learning_epochs, self.num_mini_batches = num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef = value_loss_coef, entropy_coef
        self.gamma, self.lam = gamma, lam
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.denoise_coef = float(denoise_coef)     # weight of the ActorCritic denoiser head's MSE (0: head absent / not trained)
        # True while a runner has the env store the scalar columns and bump the sampling step itself (transition_sink)
        self.env_stores_transitions = False
        self.comm_timing = None      # a list: update() appends a pair of HIP events around the wait for the gradient exchange
        # every option's state, "off" until init_storage reads the option: nobody probes for these.  The four option
        # objects (MirrorLoss, RandomNetworkDistillation, Smoothness, ValueNormalizer; None: off) and those that are on (init_storage)
        self._mirror_loss = self._rnd = self._smooth = self._guide = self._warmup = self._noise = None      # (value_normalizer: the class attribute)
        self._options = self._scalar_order = ()
        self._symmetry = self._obs_norm = None
        self._augment, self._adv_mode = False, "batch"
        self._comm, self._comm_p2p, self._comm_direct_used = None, False, False
        self._log = None      # the LogBlock behind log_block() / read_log()
        self.last_denoise_loss = None
        self._world = 1
        self._rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self._world, self._rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
            if not dist_utils.active():      # HGYM_DIST_OFF=1: this rank of a running group trains ALONE (bench.py's same-box N = 1 reference) --
                self._world = 1              # no exchange, so apply must not form a mean over ranks either

    # ------------------------------------------------------------------
    @property
    def learning_rate(self):
        return float(self.net.opt_state[self._hgym._lib.OPT_LR]) if self.net is not None else self._lr0

    @learning_rate.setter
    def learning_rate(self, v):
        self._lr0 = v
        if self.net is not None:
            self.net.opt_state[self._hgym._lib.OPT_LR] = v

    # what the last read_log() left on an option, under the names users read; None while the option is off or nothing has been read
    last_mirror_loss = property(lambda self: self._mirror_loss and self._mirror_loss.last)
    last_smoothness = property(lambda self: self._smooth and self._smooth.last)
    last_value_norm = property(lambda self: self.value_normalizer and self.value_normalizer.last)
    last_guidance = property(lambda self: self._guide and self._guide.last)

    @staticmethod
    def check_setup(num_envs, num_transitions_per_env, num_mini_batches, num_actor_obs, world=1, symmetry=None, symmetry_augmentation=True,
                    mirror_loss_coef=0.0, advantage_normalization="batch", rnd=None, smoothness=None, value_normalization=False,
                    value_normalization_eps=1e-2, guidance=None):
        """What init_storage refuses, as a function that needs no device (ValueError each), in the order the refusals win: an unknown
        advantage mode; a mirror coefficient that is negative or not finite, or one > 0 without `symmetry`; what PPO.rnd and PPO.smoothness
        refuse (their own check_setup); per-minibatch advantages over minibatches of fewer than 2 rows; value normalisation on more than one
        rank or with an eps that is negative or not finite; what PPO.guidance refuses (its own check_setup)."""
        if advantage_normalization not in PPO.ADVANTAGE_NORMALIZATIONS:
            raise ValueError("PPO.advantage_normalization=%r: one of %s" % (advantage_normalization, ", ".join(PPO.ADVANTAGE_NORMALIZATIONS)))
        coef = float(mirror_loss_coef)
        if not (coef >= 0.0 and math.isfinite(coef)):
            raise ValueError("PPO.mirror_loss_coef=%r: must be finite and >= 0" % (mirror_loss_coef,))
        if coef > 0.0 and symmetry is None:
            raise ValueError("PPO.mirror_loss_coef=%r needs the mirror tables: set PPO.symmetry to a MirrorSpec" % (mirror_loss_coef,))
        augment = symmetry is not None and bool(symmetry_augmentation)
        if rnd is not None:
            rnd_module.check_setup(world, symmetry if augment else None, augment)
        if smooth_module.parse_config(smoothness, num_actor_obs) is not None:
            # (its refusal is of the mirrored half of the storage: the mirror loss without augmentation trains on the original rows only.
            # Exactly that form is let through -- a MirrorSpec with neither half asked for is refused as it always was)
            smooth_module.check_setup(world, None if (coef > 0.0 and not augment) else symmetry)
        mb = ((2 if augment else 1) * num_envs * num_transitions_per_env) // num_mini_batches
        if advantage_normalization == "minibatch" and mb < 2:      # (rsl_rl would divide by the NaN deviation of one value)
            raise ValueError("PPO.advantage_normalization='minibatch' needs minibatches of at least 2 rows (they have %d)" % mb)
        if value_normalization:
            if int(world) > 1:      # (a follow-up: the batch statistics would go through the exchange the advantage statistics use)
                raise ValueError("PPO.value_normalization runs on one rank (world size %d): the returns' statistics have no exchange" % int(world))
            eps = float(value_normalization_eps)
            if not (eps >= 0.0 and math.isfinite(eps)):
                raise ValueError("PPO.value_normalization_eps=%r: must be finite and >= 0" % (value_normalization_eps,))
        if guide_module.parse_config(guidance) is not None:
            guide_module.check_setup(world, symmetry if (augment or coef > 0.0) else None, coef,
                                     smooth_module.parse_config(smoothness, num_actor_obs) is not None)

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        import hgym
        self._hgym = hgym
        ac = self.actor_critic
        # (PPO.check_setup by name: a subclass has refusals of its own under that name, and runs them ahead of this call)
        PPO.check_setup(num_envs, num_transitions_per_env, self.num_mini_batches, ac.num_actor_obs, self._world, self.symmetry,
                        self.symmetry_augmentation, self.mirror_loss_coef, self.advantage_normalization, self.rnd, self.smoothness,
                        bool(self.value_normalization), self.value_normalization_eps, self.guidance)
        warmup = warmup_module.parse_config(self.critic_warmup_updates)
        if warmup > 0:
            warmup_module.check_setup(self._world)
        noise = noise_module.parse_config(self.exploration_noise)
        if noise is not None:
            noise_module.check_setup(num_transitions_per_env, ac.num_actions)
        self._adv_mode = self.advantage_normalization
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, self.device)
        coef = float(self.mirror_loss_coef)
        self._augment = self.symmetry is not None and bool(self.symmetry_augmentation)
        self._symmetry = self.symmetry if (self._augment or coef > 0.0) else None      # neither half asked for: symmetry off
        if self._symmetry is not None:
            self.storage.enable_mirror(self._symmetry)      # (before enable_shadow and before anything binds a slot's address)
        mb = ((2 if self._augment else 1) * num_envs * num_transitions_per_env) // self.num_mini_batches
        if self._adv_mode == "minibatch":
            self.storage.enable_minibatch_advantages(self.num_mini_batches, mb)      # (behind enable_mirror: the enlarged column's layout)
        aux = getattr(ac, "denoiser_hidden_dims", None)
        cfg = hgym.make_net_config(ac.num_actor_obs, ac.num_critic_obs, ac.num_actions, ac.actor_hidden_dims, ac.critic_hidden_dims,
                                   self.precision, max(mb, num_envs), aux_hidden=aux, aux_out=getattr(ac, "denoiser_targets", 0),
                                   aux_target_offset=ac.num_critic_obs - getattr(ac, "denoiser_targets", 0),
                                   activation=getattr(ac, "activation", None), fused_activation=getattr(ac, "fused_activation", False),
                                   noise_std_type=getattr(ac, "noise_std_type", "scalar"))
        # data-parallel update: the exchange is chosen here, once (HGYM_COMM=auto: the direct kernel over peer mappings is set up,
        # checked and timed against the collective, and used when it is faster; any failure falls back on every rank -- dist_utils).
        # With the direct exchange the gradient vector lives in peer-mapped memory.
        self._comm = dist_utils.make_comm(int(hgym._lib.lib.hgym_net_param_count(C.byref(cfg))) + 1, self.device)
        self._comm_p2p = self._comm is not None and dist_utils.comm_backend() == "p2p"
        self._comm_pin = None
        self.comm_report = dist_utils.comm_report()     # mode, used, fallback_reason, probe timings (bench.py prints it)
        self._comm_direct_used = False      # the direct kernel has carried at least one real gradient (also under HGYM_COMM=both)
        self.comm_flip = False      # bench.py: use the OTHER exchange for the next update() (timing both in its profiling iterations)
        # empirical observation normalisation (ActorCritic(empirical_normalization=True)): the net owns the statistics and folds them into
        # the first layers; update() unfolds every minibatch gradient and ends with the normaliser step
        self._obs_norm = getattr(ac, "obs_norm_spec", None)
        self.net = hgym.NetBuffers(cfg, self.device, learning_rate=self._lr0, grads_ext=None if self._comm is None else self._comm.data,
                                   obs_norm=self._obs_norm)
        dist_utils.broadcast_parameters(ac.parameters())   # identical initial parameters on every rank
        ac.bind(self.net)
        # bf16 shadows of the stored observation rows: the policy launches leave them behind, the update gathers from them
        # (environment knobs are read ONCE, here: a captured rollout graph keeps whatever was active at capture)
        self._check_shadow = os.environ.get("HGYM_CHECK_SHADOW", "0") == "1"
        if os.environ.get("HGYM_SHADOW", "1") != "0":
            self.storage.enable_shadow(self.net.shadow_ld(0), self.net.shadow_ld(1))
        self._ppo_cfg = hgym.make_ppo_config(self.clip_param, self.value_loss_coef, self.entropy_coef, self.max_grad_norm,
                                             self.desired_kl if self.desired_kl is not None else 0.0,
                                             adaptive=(self.desired_kl is not None and self.schedule == "adaptive"),
                                             world_size=self._world,
                                             # update() applies exactly what hgym_ppo_grad produced -- unless the unfold of a normalised
                                             # net comes between the two: the norm is then taken by hgym_ppo_apply's own pass
                                             grad_norm_ready=self._obs_norm is None,
                                             aux_coef=self.denoise_coef if aux else 0.0,
                                             clipped_value_loss=self.use_clipped_value_loss, mirror_coef=coef)
        if coef > 0.0:      # the pre-pass's output (one minibatch of raw partner means) and the two sums behind the per-update loss sums
            self._mirror_loss = MirrorLoss(coef, mb, ac.num_actions, self.device)
        smooth = smooth_module.parse_config(self.smoothness, ac.num_actor_obs, torch.initial_seed())
        if smooth is not None:      # the successor map of a whole permutation, the two pre-passes' outputs, the perturbed rows, the four sums
            if coef > 0.0 and smooth["spatial_coef"] > 0.0:      # a perturbation that told left from right would fight the mirror term
                smooth_module.check_noise_mirror(smooth["noise_std"], self._symmetry.obs_src)
            self._smooth = smooth_module.Smoothness(smooth, self.num_mini_batches * mb, mb, ac.num_actor_obs, ac.num_actions, self.device,
                                                    mirror_loss=coef > 0.0)
        self._sample_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._perm_seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0xABCD + 104729 * self._rank) & 0xFFFFFFFFFFFFFFFF
        self._perm_draws = 0
        self._deferred_ready = False        # deferred_values() has run since the last compute_returns()
        self._slot_T_written = False        # the rollout's producer writes the NEXT observations into the storage's slots (read by PPO.rnd)
        # diagnostics(): slot 0 of the observations as the update saw it (diagnostics_prepare), whether an update has run on the stored rows
        self._diag_rows0 = None
        self._diag_saved = self._diag_updated = False
        self._diag_block = None
        self._perm_draws_dev = torch.zeros(1, dtype=torch.int64, device=self.device)      # the same number where a captured update reads it
        ac._sample_step = self._sample_step
        # exploration-noise key: from the run's seed (as the permutation key above) and the rank
        ac._sample_seed = (torch.initial_seed() * 0xD1342543DE82EF95 + 0x5EED + 7919 * self._rank) & 0xFFFFFFFFFFFFFFFF
        if noise is not None:      # the filter, the AR(1) state (seeded like the key above), the table of one rollout
            self._noise = noise_module.ExplorationNoise(noise, num_transitions_per_env, num_envs, ac.num_actions, self.device,
                                                        seed=ac._sample_seed ^ 0xA5A5A5A5A5A5A5A5)
        if self.rnd is not None:      # two more NetBuffers at the PPO precision, the reward pass's block, the storage's rnd_* fields
            self._rnd = self.rnd.bind(int(self.net.cfg.precision), max(mb, 1), self.device, num_envs)
            self.storage.enable_rnd(self._rnd.num_states, self._rnd.num_outputs)
        if self.value_normalization:      # the block of three doubles, the merge's scratch, the bootstrap value's buffer
            self.value_normalizer = ValueNormalizer.on_device(self.value_normalization_eps, num_envs * num_transitions_per_env, num_envs, self.device)
        guide = guide_module.parse_config(self.guidance)
        if guide is not None:      # the teacher's NetBuffers, the device count and coefficient, the log's three doubles, storage.teacher_mu
            self._guide = guide_module.Guidance(guide, ac, self.net, num_envs * num_transitions_per_env, self.device)
            self.storage.enable_guidance(ac.num_actions)
            self._guide.bind_storage(self.storage)
        if warmup > 0:      # the value-loss and apply configurations of the critic-only updates, the log's three doubles
            self._warmup = warmup_module.CriticWarmup(warmup, self._ppo_cfg, self.clip_param, self.value_loss_coef,
                                                      bool(self.use_clipped_value_loss), self.device)
        # the options that are on, in the two orders that are fixed: the log block's byte layout (checkpoints, tools and tests hold such
        # blocks) and the order in which the writer gets their scalars.  A new option goes at the end of both.
        on = lambda *options: tuple(o for o in options if o is not None)
        self._options = on(self._mirror_loss, self._rnd, self._smooth, self.value_normalizer, self._guide, self._warmup)
        self._scalar_order = on(self._mirror_loss, self._smooth, self._rnd, self.value_normalizer, self._guide, self._warmup)
        if self._noise is not None:      # (nothing in the update sees it: no log part, no entry in update_graph_key -- rollout_graph_key has it)
            self._scalar_order += (self._noise,)
        self._log = LogBlock(self._log_parts())

    def _log_parts(self):
        """opt | mirror(2) | rnd_sums(2) | rnd_block(RND_HEADER) | smooth(4) | value_norm(3) | guide(2) | guide_coef(1) | critic_warmup(3): opt_state, then the part(s) of every option that
        is on; value_norm is the statistics' block itself (count, mean, var)."""
        return [("opt", self.net.opt_state)] + [part for o in self._options for part in o.log_parts()]

    def seek(self, iteration, steps_per_iteration):
        """Position the device generators' counters where a run that has done `iteration` learning iterations has them
        (OnPolicyRunner.load): a resumed run continues the exploration-noise and permutation streams instead of replaying them
        from the start.  The reference's checkpoint carries no generator state (on_policy_runner.py:274-281); the counters are
        functions of the iteration number, so neither does this one.  (The env's own draw streams are positioned by
        LeggedRobot.seek, which the runner calls next to this.)"""
        self._sample_step.fill_(int(iteration) * int(steps_per_iteration))
        self._perm_draws = int(iteration)
        with torch.inference_mode():
            self._perm_draws_dev.fill_(int(iteration))

    def check_comm(self, words=None):
        """The direct exchange's status word, read where the host synchronises anyway (the end of a synchronous update, the end of
        learn(), the asynchronous log's snapshot): raises dist_utils.CommTimeout if a bounded wait of any call expired -- that
        minibatch's gradient was garbage and the replicas have diverged, so training must not go on silently.  words: a host copy
        of the status block taken earlier (comm_status_snapshot); None: synchronise and read it now."""
        if self._comm is None or not (self._comm_p2p or self._comm_direct_used):      # (HGYM_COMM=both: bench.py's comm_flip updates ran it)
            return
        self._comm.raise_if_expired(self._comm.read_status() if words is None else words)

    def comm_status_snapshot(self, slot):
        """Stream-ordered device -> pinned-host copy of the status block (no host wait); the caller reads it after its own event."""
        if self._comm is None or not (self._comm_p2p or self._comm_direct_used):
            return None
        if self._comm_pin is None:
            self._comm_pin = [torch.zeros(16, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._comm_pin[slot].copy_(self._comm.status, non_blocking=True)
        return self._comm_pin[slot]

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    # ------------------------------------------------------------------ rollout
    def act(self, obs, critic_obs, env_fin=None):
        """env_fin (native extension): a postponed env-step finaliser to run inside this policy launch
        (LeggedRobot.take_pending_finalize)."""
        st, s = self.storage, self.storage.step
        self._rows_overwritten()
        out = None
        if s < st.num_transitions_per_env:     # write straight into the storage slot (no add_transitions copies)
            out = dict(actions=st.actions[s], mu=st.mu[s], sigma=st.sigma[s], logp=st.actions_log_prob[s].view(-1), values=st.values[s])
        t = self.transition
        # the slot's bf16 shadow only when `obs` IS the slot (the zero-copy runner): a copy made later by add_transitions
        # invalidates it again
        sh = st.shadow_slot(s) if (out is not None and obs.data_ptr() == st._obs_all[s].data_ptr()
                                   and st._priv_all is not None and critic_obs.data_ptr() == st._priv_all[s].data_ptr()) else None
        # obs IS the slot: a zero-copy rollout, whose env writes step s + 1's observations into slot s + 1 -- at the last step, slot T
        self._slot_T_written = out is not None and obs.data_ptr() == st._obs_all[s].data_ptr()
        z = None
        if self._noise is not None:      # the rollout's table at its first step (the sampling step is read on the device), then this step's row
            # (every act() at storage.step == 0 fills all T rows and moves the AR(1) state on by T steps: a second call there, or a
            # stepwise rollout that stops early, leaves the state ahead of the steps taken -- still a draw of the stationary process)
            if s == 0:
                self._noise.fill(self._sample_step, self.actor_critic._sample_seed)
            z = self._noise.row(s) if s < st.num_transitions_per_env else None
        t.actions = self.actor_critic.act(obs, critic_obs, out=out, env_fin=env_fin, shadow=sh, z=z)
        last = self.actor_critic._last
        t.values, t.actions_log_prob = last["values"], last["logp"]
        if self.value_normalizer is not None:
            # the critic's output -> a raw value, in place, before anything reads the slot: hgym_store_step, the env's transition sink, the
            # finaliser riding in the next policy launch (time-out bootstrap r += gamma V), GAE
            self.value_normalizer.denormalize(t.values)
        t.action_mean, t.action_sigma = last["mu"], last["sigma"]
        t.observations, t.critic_observations = obs, critic_obs
        if not self.env_stores_transitions:
            self._sample_step += 1
        return t.actions

    def rollout_columns(self, deferred):
        """The storage's slot columns a fused rollout fills (LeggedRobot.rollout_begin): launch i reads slot i of the observations,
        writes slot i + 1 and the policy's outputs of slot i; its finaliser stores rewards / dones of slot i (time-out bootstrap
        included).  deferred: no values column -- slot i receives the RAW reward and the bootstrap's time-out flags, and
        deferred_values() fills storage.values and has compute_returns apply the bootstrap."""
        st = self.storage
        if deferred:
            st.enable_deferred_values()
        return dict(obs=st._obs_all, priv=st._priv_all, actions=st.actions, mu=st.mu, sigma=st.sigma, logp=st.actions_log_prob,
                    values=None if deferred else st.values, rewards=st.rewards, dones=st.dones, time_outs=st.time_outs if deferred else None,
                    obs_bf16=st._obs_bf16, priv_bf16=st._priv_bf16, step=self._sample_step, gamma=self.gamma,
                    seed=self.actor_critic._sample_seed, z=None if self._noise is None else self._noise.table)

    def _rows_overwritten(self):      # a rollout is writing the rows diagnostics() would read
        self._diag_saved = self._diag_updated = False

    def _rollout_done(self, step, shadow_valid, deferred_ready):
        """The host state a finished rollout leaves: fused launches and replays of any form write it here, the stepwise calls piece by piece."""
        self.storage.step, self.storage.shadow_valid, self._deferred_ready = step, list(shadow_valid), deferred_ready
        self._rows_overwritten()

    def rollout_end_state(self):      # _rollout_done()'s arguments as the rollout that has just run left them: a captured rollout holds them for its replays
        return self.storage.step, list(self.storage.shadow_valid), self._deferred_ready

    def fused_rollout_step(self, env, T=None, deferred=False, rows_ahead=None, l0_ahead=None):
        """All T fused rollout steps: act() + env.step() + process_env_step() as ONE launch each (LeggedRobot.rollout_step) into
        storage slots 0 .. T (default: the whole storage).  deferred: see rollout_columns; the caller follows with deferred_values(),
        which ends the rollout.  rows_ahead / l0_ahead: None = the env's HGYM_ROWS_AHEAD / HGYM_L0_AHEAD (LeggedRobot.rollout_begin)."""
        st = self.storage
        T = st.num_transitions_per_env if T is None else int(T)
        if st.step != 0 or T > st.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        self._rows_overwritten()
        self._slot_T_written = True      # launch i writes slot i + 1
        if self._noise is not None:      # the T rows the launches read, ahead of the first (the same sampling step hgym_rollout_begin reads)
            self._noise.fill(self._sample_step, self.actor_critic._sample_seed, T)
        env.rollout_begin(self.net, self.rollout_columns(deferred), T, rows_ahead, l0_ahead)
        for i in range(T):
            env.rollout_step(i)
        env.rollout_end()
        if not deferred:      # each launch wrote its slot's shadows
            self._rollout_done(T, [True] * T + st.shadow_valid[T:] if st._obs_bf16 is not None else st.shadow_valid, self._deferred_ready)

    def transition_sink(self):
        """The scalar columns of the storage slot act() has just filled, for an env that can store them itself
        (LeggedRobot.bind_transition); the caller sets `env_stores_transitions` for the duration and follows env.step
        with process_env_step(..., stored=True)."""
        st, s = self.storage, self.storage.step
        return dict(values=st.values[s], rewards=st.rewards[s], dones=st.dones[s], step=self._sample_step, gamma=self.gamma)

    def process_env_step(self, rewards, dones, infos, stored=False):
        """`stored=True`: the env already wrote this step's rewards / dones slot (transition_sink)."""
        L = self._hgym._lib
        st, s = self.storage, self.storage.step
        if s >= st.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        if not stored:
            to = infos.get("time_outs") if isinstance(infos, dict) else None
            d8 = dones if dones.dtype == torch.uint8 else dones.view(torch.uint8) if dones.dtype == torch.bool else dones.to(torch.uint8)
            t8 = None if to is None else (to.view(torch.uint8) if to.dtype == torch.bool else to.to(torch.uint8))
            L.check(L.lib.hgym_store_step(st.num_envs, L.fptr(rewards), L.fptr(self.transition.values), L.u8ptr(t8), L.u8ptr(d8),
                                          self.gamma, L.fptr(st.rewards[s]), L.u8ptr(st.dones[s]),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_store_step")
        self.transition.rewards = st.rewards[s].view(-1)
        self.transition.dones = st.dones[s].view(-1)
        st.add_transitions(self.transition)
        self.transition.clear()
        self.actor_critic.reset(dones)

    def deferred_values(self):
        """After a fused_rollout_step(deferred=True): ActorCritic.evaluate over EVERY stored privileged row in one
        pass (the T slots -> storage.values, the bootstrap observation in slot T -> storage.last_values), 64-row tiles at the update's
        efficiency instead of T + 1 latency-bound launches; the tiles also leave the bf16 shadow of the rows they read.  The
        reference evaluates V(s_t) inside PPO.act (ppo.py:96, on_policy_runner.py:129) -- same weights (they do not change during
        collection), same rows, same kernel arithmetic."""
        st = self.storage
        T, N = st.num_transitions_per_env, st.num_envs
        shadow = st._priv_bf16.flatten(0, 1) if st._priv_bf16 is not None else None
        self.net.critic_values(st._priv_all[:T].flatten(0, 1), st.values.view(-1), shadow)
        self.net.critic_values(st._priv_all[T], st.last_values.view(-1))
        if self.value_normalizer is not None:      # the statistics the critic was last trained under: those of the previous update
            self.value_normalizer.denormalize(st.values)
            self.value_normalizer.denormalize(st.last_values)
        self._rollout_done(T, [True] * T if shadow is not None else st.shadow_valid, True)

    def _adv_stats(self, stats):
        """(sum adv, sum adv^2, count) of this rank's shard -> of the global batch, in place: through the direct exchange's mappings when that
        is what the gradients use (hgym_comm_sum64: rank-ordered fp64 sum, no torch.distributed call -- the update stays capturable), else
        the collective."""
        if dist_utils.active() and self._comm is not None and self._comm_p2p and not self.comm_flip:
            self._comm.sum64(stats)
            return stats
        return dist_utils.allreduce_adv_stats(stats)

    def compute_returns(self, last_critic_obs, last_obs=None):
        """last_obs (native extension, read by PPO.rnd only): the env's observations behind the last step, for an RND state taken from
        "obs" when the rollout did not write the storage's slot T (RandomNetworkDistillation.reward_pass)."""
        st, deferred = self.storage, self._deferred_ready       # deferred_values() has evaluated the bootstrap observation with the rest
        last_values = st.last_values if deferred else self.actor_critic.evaluate(last_critic_obs)
        vn = self.value_normalizer
        if vn is not None and not deferred:      # (deferred_values() has denormalised its own)
            last_values = vn.denormalize(last_values.reshape(-1, 1).contiguous(), out=vn.last_values).view(-1, 1)
        if self._smooth is not None and self._smooth.cfg["temporal_coef"] > 0.0 and not self._slot_T_written:
            # a rollout that copied its observations in (add_transitions) has not written slot T: the temporal term's successor of the last
            # step's rows is the bootstrap observation, which only the caller holds
            if last_obs is None:
                raise RuntimeError("PPO.smoothness: the rollout did not write the storage's slot T; call compute_returns(last_critic_obs, "
                                   "last_obs=<the env's last observations>)")
            st._obs_all[st.num_transitions_per_env].copy_(last_obs)
        if self._rnd is not None:      # rewards += intrinsic, ahead of GAE on both paths (the deferred path's time-out bootstrap is added behind it)
            self._rnd.reward_pass(st, last_critic_obs, last_obs, self._slot_T_written)
        st.compute_returns(last_values, self.gamma, self.lam, stats_hook=self._adv_stats, time_outs=st.time_outs if deferred else None,
                           normalize=self._adv_mode == "batch")
        if vn is not None:      # merge the raw returns FIRST, then returns and old values into the critic's units under the new statistics
            vn.normalize_targets(st.returns, st.values)
        warming = self._warmup is not None and self._warmup.active      # critic-only: no actor-side option is invoked
        if self._warmup is not None:
            self._warmup.retire_if_done()        # (once, and never inside a capture)
        if self._guide is not None:
            self._guide.retire_if_run_out()      # (once, and never inside a capture)
            if self._guide.active and not warming:      # the teacher's mean of the T N stored rows, for every minibatch of every epoch
                self._guide.teacher_pass(st)
        self._returns_done()

    def _returns_done(self):      # what compute_returns() changes on the host, issued or replayed: the deferred values are used up
        self._deferred_ready = False

    # ------------------------------------------------------------------ update
    def update_capturable(self):
        """True when compute_returns() + update(sync=False) enqueue the same launches with the same arguments in every iteration, i.e. may
        be captured into a HIP graph and replayed (OnPolicyRunner): the device permutation (its draw number is read on the device), no
        timing probes inside the update, and either one rank or the direct gradient exchange with its call number on the device -- a
        torch.distributed collective (RCCL / gloo) stays eager."""
        if self.permutation != "device" or self.comm_timing is not None or self._check_shadow:
            return False
        if not dist_utils.active():
            return True
        if self._obs_norm is not None:      # the normaliser's sums go through a torch.distributed all-reduce: eager
            return False
        return bool(self._comm is not None and self._comm_p2p and not self.comm_flip and getattr(self._comm, "capturable", False))

    def update_graph_key(self):
        """Everything host-side that compute_returns() / update() bake into their launches, as (name, value) pairs: a change re-captures.
        dict(key)[name] reads an entry; an option's entries are listed here as they read while it is off, and an option that is on
        fills in its own (its graph_key())."""
        st = self.storage
        key = dict(ppo_cfg=_struct_bytes(self._ppo_cfg), num_learning_epochs=self.num_learning_epochs, num_mini_batches=self.num_mini_batches,
                   gamma=float(self.gamma), lam=float(self.lam), permutation=self.permutation, perm_seed=self._perm_seed, storage=id(st),
                   net=id(self.net), dist_active=bool(dist_utils.active()), comm_p2p=bool(self._comm_p2p), net_cfg=_struct_bytes(self.net.cfg),
                   shadows=st._obs_bf16 is not None, comm_flip=bool(self.comm_flip), world=self._world,
                   symmetry=None if self._symmetry is None else self._symmetry.key(),
                   # (the mirror loss's coefficient is also part of ppo_cfg's bytes; augment: whether the batch is doubled)
                   mirror_coef=0.0, augment=self._augment, mirror_scratch=None, smoothness=None, rnd=None,
                   adv_mode=self._adv_mode, adv_scratch=st.minibatch_advantages_key(), obs_norm=self._obs_norm, value_norm=None,
                   critic_warmup=False, guidance=None)
        for o in self._options:
            key.update(o.graph_key())
        return tuple(key.items())

    def rollout_graph_key(self):
        """Everything of this side that a rollout bakes into its launches: the storage's slots, the sink's gamma (BY VALUE), the shadows."""
        key = id(self.storage), self.gamma, self.storage._obs_bf16 is not None
        # with value normalisation the stepwise rollout contains the denormalise launches (eps by value, the block by address); off: the key as ever
        key = key if self.value_normalizer is None else key + (self.value_normalizer.graph_key()["value_norm"],)
        # with exploration noise the rollout contains the table launch and its launches read the table's rows; off: the key as ever
        return key if self._noise is None else key + (self._noise.graph_key(),)

    def after_rollout_replay(self, end_state):
        """Host-side book-keeping of one replayed rollout.  end_state: rollout_end_state() behind the captured pass."""
        self._rollout_done(*end_state)

    def after_update_replay(self):
        """Host-side book-keeping of one replayed compute_returns() + update(sync=False)."""
        self._returns_done()
        self._update_done()

    def _direct_exchange(self):      # this update's gradient exchange is the direct kernel (comm_flip: not the one init_storage chose)
        return dist_utils.active() and self._comm is not None and self._comm_p2p != bool(self.comm_flip)

    def _update_done(self):      # what update() changes on the host besides enqueueing work, issued or replayed (an update that raises part-way has not run it)
        if self.permutation == "device":
            self._perm_draws += 1
        self.storage.cleared()
        self._diag_updated = True
        if self._direct_exchange():
            self._comm_direct_used = True
        if self._warmup is not None and self._warmup.active:
            self._warmup.update_done()           # (a critic-only update: guidance's schedule count stays where it is)
        elif self._guide is not None:
            self._guide.update_done()

    def update(self, sync=True):
        """ppo.py:119-184.  Returns (mean_value_loss, mean_surrogate_loss) as floats -- the one host read-back of the
        update.  sync=False (native extension, used by the runner when nothing is logged): no read-back, returns
        (None, None), so the host can already enqueue the next rollout while this update runs."""
        hgym, net, st, direct = self._hgym, self.net, self.storage, self._direct_exchange()
        T, N = st.num_transitions_per_env, st.num_envs
        sym, aug, mirror_loss, smooth = self._symmetry is not None, self._augment, self._mirror_loss, self._smooth
        guide = self._guide if (self._guide is not None and self._guide.active) else None      # (run out: the plain update)
        warm = self._warmup if (self._warmup is not None and self._warmup.active) else None     # critic-only: hgym_vf_grad in place of hgym_ppo_grad*
        if warm is not None:
            mirror_loss = smooth = guide = None      # the actor-side options are not invoked
        if sym:
            # the mirrored half of every column, from the finished rollout (returns, advantages, values, shadows: all there); the mirror
            # loss alone reads only the mirrored observations
            st.mirror(observations_only=not aug)
        batch = (2 if aug else 1) * T * N
        mb = batch // self.num_mini_batches
        # one permutation for every epoch (rollout_storage.py:149,165-170)
        if self.permutation == "device":
            # the draw number lives on the device as well: the launch reads it there, so a captured update (OnPolicyRunner's second HIP
            # graph) draws a NEW permutation at every replay.  Eager calls re-seat the device copy from the host count first (the host
            # count is what seek() / a checkpoint resume set); under capture nothing is re-seated -- replays continue the device count.
            # The host's is advanced by _update_done().
            with torch.inference_mode():        # (the counter may have been created under the runner's inference mode)
                if not torch.cuda.is_current_stream_capturing():
                    self._perm_draws_dev.fill_(self._perm_draws)
                self._perm_draws_dev.add_(1)
            perm = st.permutation(self.num_mini_batches * mb, self._perm_seed, self._perm_draws_dev)
        else:
            perm = torch.randperm(self.num_mini_batches * mb, device=self.device)
        if aug:
            perm = st.mirror_index(perm)      # drawn over 2 T N rows; the mirrored half lies behind the bootstrap slot
        if mirror_loss is not None:      # every drawn row's partner, for every epoch
            pair = mirror_loss.begin_update(perm, st)
        if smooth is not None:      # one pass over the whole permutation
            smooth.begin_update(perm, st)
        cols = st.batch_columns()
        if smooth is not None:      # the T + 1 observation slots are ONE allocation under the column's base pointer: next_idx reaches into slot T
            assert cols[0].data_ptr() == st._obs_all.data_ptr() and st._obs_all.is_contiguous()
        if self._adv_mode == "minibatch":
            # the slices below partition perm once for every epoch: all minibatches standardised in one pass, into the column the batches name
            cols = cols[:4] + (st.normalize_minibatch_advantages(perm, self.num_mini_batches),) + cols[5:]
        sh = st.shadows(mirrored=sym)
        if sh is not None and self._check_shadow:
            st.check_shadows()
        sh = dict(obs_bf16=sh[0], priv_bf16=sh[1]) if sh is not None else {}
        net.opt_state[hgym._lib.OPT_KL_SUM:hgym._lib.OPT_MINIBATCHES + 1] = 0.0     # the four per-update sums and their count (and the informational last norm between them): one fill
        if self._ppo_cfg.aux_coef > 0.0:
            net.opt_state[hgym._lib.OPT_AUX_SUM:hgym._lib.OPT_AUX_SUM + 1] = 0.0     # (a slice: a fill kernel -- an indexed scalar store is a host-to-device copy, which a stream capture refuses)
        if self._rnd is not None:
            self._rnd.begin_update()
        if guide is not None:      # this update's coefficient, formed on the device; the two sums zeroed
            guide.begin_update()
            guided = guide.minibatch()      # (the same descriptor for every minibatch: the column is gathered through the batch's idx)
        if warm is not None:       # the two sums zeroed, the log's count moved on
            warm.begin_update()
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                idx = perm[i * mb:(i + 1) * mb]
                if warm is not None:      # the critic alone: its gradient, +0.0 everywhere else, then the step with the learning-rate rule off
                    net.vf_grad(warm.vf_cfg, hgym.make_vf_batch(cols[1], cols[3], cols[5], idx, priv_bf16=sh.get("priv_bf16")), warm.sums)
                    if self._obs_norm is not None:
                        net.norm_unfold_grad()
                    net.ppo_apply(warm.apply_cfg)
                    if self._rnd is not None:
                        self._rnd.train_step(st, idx)
                    continue
                mirror = {} if mirror_loss is None else mirror_loss.minibatch(pair[i * mb:(i + 1) * mb], st)
                batch = hgym.make_batch(*cols, idx, **mirror, **sh)
                if smooth is not None and mirror_loss is not None:      # one actor head for the three detached-target terms
                    net.ppo_grad_smooth_mirror(self._ppo_cfg, batch, smooth.minibatch(i), smooth.head_partials)
                elif smooth is not None:
                    net.ppo_grad_smooth(self._ppo_cfg, batch, smooth.minibatch(i))
                elif guide is not None:
                    net.ppo_grad_guide(self._ppo_cfg, batch, guided)
                else:
                    net.ppo_grad(self._ppo_cfg, batch)
                if self._obs_norm is not None:
                    net.norm_unfold_grad()      # first-layer gradients: of the folded operands -> of the master parameters, ahead of the exchange and the norm
                if dist_utils.active():
                    # ONE bucket, [flat gradient | KL]: nothing of this minibatch is left to run under the exchange (apply needs it),
                    # and two buckets pay the collective's latency twice.  (Rounds 1-2 split the weight-gradient launch in two so that
                    # the actor's bucket travelled under the critic's products: the two half-empty launches cost 106 us more per
                    # minibatch than the one launch -- more than the exchange they hid; profiles/r03_grad_parts_ab.txt.)
                    probe = self.comm_timing is not None
                    h = None if direct else dist_utils.start_sum(net.grads_ext)
                    if probe:       # (behind the collective's start: the pair times the wait)
                        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                        ev[0].record()
                    if direct:      # HGYM_COMM=p2p: one kernel on this stream (reduce-scatter + all-gather over the peer mappings)
                        self._comm.allreduce()
                    else:
                        dist_utils.finish(h)
                    if probe:
                        ev[1].record()
                        self.comm_timing.append(ev + ("p2p" if direct else "collective",))
                net.ppo_apply(self._ppo_cfg)
                if self._rnd is not None:      # one predictor step on the SAME rows, against the target's embedding of them
                    self._rnd.train_step(st, idx)
        if self._obs_norm is not None:
            self.normalizer_step()
        if self._rnd is not None:
            self._rnd.end_update(st)
        st.rotate()
        self._update_done()
        if not sync:
            return None, None
        block = self.log_block().cpu()         # the one host read-back of the update
        self.check_comm()                      # (the stream is idle now: reading the exchange's status costs one small copy)
        o = self.read_log(block)
        return o["mean_value_loss"], o["mean_surrogate_loss"]

    def log_block(self):
        """What a log line reads after an update, as ONE device tensor (one copy to the host): the parts init_storage listed
        (_log_parts); opt_state itself when no option adds a part."""
        return self._log.device()

    def read_log(self, block):
        """A host copy of log_block() -> hgym.opt_summary's dict; sets last_denoise_loss, last_mirror_loss, last_smoothness,
        last_value_norm, last_guidance and RND's last_log on the way.  The one reader behind update(sync=True) and the runner's asynchronous log."""
        parts = self._log.split(block)
        for option in self._options:      # each leaves its numbers on itself: last_mirror_loss, last_smoothness, last_value_norm read them there
            option.read_log(parts)
        o = self._hgym.opt_summary(parts["opt"], self._ppo_cfg.aux_coef > 0.0)
        self.last_denoise_loss = o["denoise_loss"]
        if self._warmup is not None and self._warmup.last["trained"]:      # a critic-only update: its value loss, no surrogate
            o = dict(o, mean_value_loss=self._warmup.last["value_loss"], mean_surrogate_loss=0.0)
        return o

    def log_scalars(self):
        """The optional loss scalars of the last read_log() as ordered (tag, value) pairs, for the runner's writer."""
        out = []
        if self.denoise_coef and self.last_denoise_loss is not None:
            out.append(("Loss/denoise_mse", self.last_denoise_loss))
        for option in self._scalar_order:      # Loss/mirror; Loss/smooth_temporal, Loss/smooth_spatial; Loss/rnd, Rnd/*; Policy/value_norm_mean, Policy/value_norm_std; Loss/guidance, Guidance/coef
            out += option.log_scalars()
        return out

    def normalizer_step(self):
        """The normaliser's one step per iteration, at the end of update(), ahead of storage.clear(): accumulate the T * N stored raw
        rows of both kinds (slots 0 .. T - 1; with symmetry on the original rows only -- the mirrored copies lie behind the bootstrap
        slot), merge them into the running statistics, refold the first layers.  The statistics are therefore frozen while a rollout is
        collected and while its update runs: the stored mu, sigma and log-probabilities stay those of the net the update
        differentiates.  (rsl_rl merges at every env step.)  Several ranks: the raw fp64 sums pass through one all-reduce before the
        merge, so every rank merges the global batch into the same state.  The launches and their arguments are the same in every
        iteration: on one rank the step is part of the captured update."""
        st, net = self.storage, self.net
        T, N = st.num_transitions_per_env, st.num_envs
        obs = st._obs_all[:T].flatten(0, 1)
        priv = (st._priv_all if st._priv_all is not None else st._obs_all)[:T].flatten(0, 1)
        net.norm_accumulate(obs, priv)
        if dist_utils.active():
            torch.distributed.all_reduce(net.norm_view("sums"))
        net.norm_merge()

    # ------------------------------------------------------------------ diagnostics of an update
    def diagnostics_prepare(self):
        """Call between a rollout and the update() (or its graph replay) that diagnostics() is to follow.  update() ends with
        storage.clear(), which copies the bootstrap observation (slot T) over slot 0: of everything the update trains on, the N
        observation rows of slot 0 are the one thing the storage no longer holds afterwards.  This keeps them: two device copies
        (N x (num_obs + num_priv) floats) on the current stream, outside both HIP graphs; nothing else changes."""
        st = self.storage
        with torch.inference_mode():
            if self._diag_rows0 is None:
                self._diag_rows0 = (torch.empty_like(st._obs_all[0]), None if st._priv_all is None else torch.empty_like(st._priv_all[0]))
            self._diag_rows0[0].copy_(st._obs_all[0])
            if st._priv_all is not None:
                self._diag_rows0[1].copy_(st._priv_all[0])
        self._diag_saved, self._diag_updated = True, False

    def diagnostics(self, sync=True):
        """What the last update did to the policy, measured on the T * N rows it trained on: the UPDATED actor and critic are evaluated
        once more on the stored observations and the result is reduced on the device against the stored actions, old mu / sigma /
        log-probability / values, returns and advantages (hgym_ppo_diagnostics: fp64 sums in a fixed order, the same bits in every run).

        Valid after diagnostics_prepare() + update() and before the next rollout writes slot 0; RuntimeError otherwise.  Around the pass
        slot 0 of the observations holds the saved rows again and is then re-filled from slot T, as clear() left it: the next rollout
        reads the same bits.  Parameters, gradients, Adam's state, opt_state, the bf16 shadows and every storage column are left alone.

        sync=True: the dict of python floats of hgym.diag_from_block (samples, clip_fraction, kl, approx_kl, ratio_mean / _max / _min,
        surrogate, entropy, value_clip_fraction, return_mean, return_std, explained_variance, explained_variance_new, value_rmse,
        value_rmse_new) -- one read-back.  sync=False: the device block (its first 16 doubles are the sums), nothing read back: the
        runner copies it into a pinned slot behind the update.  May be called again: same rows, same bits.

        `kl` is the exact KL(old || new) of the two Gaussians, averaged over the WHOLE batch after the LAST minibatch step; the
        learning-rate rule sees one minibatch at a time, before its step, and its expression carries + 1e-5 inside the logarithm.

        `surrogate` is formed with the advantages the update trained on (PPO.advantage_normalization): the batch-standardised column by
        default; under "minibatch" storage.advantages_mb -- every original row standardised by the statistics of the minibatch that drew
        it, and 0 for a row no minibatch drew (batch % num_mini_batches != 0), which then adds nothing to the sum; under "none" the raw
        returns - values, so its scale is the rewards'.

        Data-parallel runs: every rank reports its own shard of the batch; no collective is added."""
        st = self.storage
        if st is None or not self._diag_updated:
            raise RuntimeError("PPO.diagnostics(): no update() has run on the rows in the storage (call it after update(), before the next rollout)")
        if st.step != 0:
            raise RuntimeError("PPO.diagnostics(): the storage is being filled again (storage.step = %d)" % st.step)
        if not self._diag_saved:
            raise RuntimeError("PPO.diagnostics(): call diagnostics_prepare() between the rollout and update() -- update() ends with "
                               "storage.clear(), which overwrites the observations of slot 0 with the bootstrap observation")
        T, N = st.num_transitions_per_env, st.num_envs
        L = self._hgym._lib
        fl = lambda t: t.flatten(0, 1)
        with torch.inference_mode():
            if self._diag_block is None:
                self._diag_block = L.diag_block(T * N, self.device)
            st._obs_all[0].copy_(self._diag_rows0[0])
            if st._priv_all is not None:
                st._priv_all[0].copy_(self._diag_rows0[1])
            obs = fl(st.observations)
            priv = fl(st.privileged_observations) if st.privileged_observations is not None else obs
            adv = st.advantages_mb[:T * N] if self._adv_mode == "minibatch" else st.advantages.view(-1)      # the column the update trained on
            cols = (obs, priv, fl(st.actions), st.values.view(-1), adv, st.returns.view(-1),
                    st.actions_log_prob.view(-1), fl(st.mu), fl(st.sigma))
            self.net.ppo_diagnostics(self._ppo_cfg, cols, self._diag_block)
            st._obs_all[0].copy_(st._obs_all[T])
            if st._priv_all is not None:
                st._priv_all[0].copy_(st._priv_all[T])
        if not sync:
            return self._diag_block
        return self._hgym.diag_from_block(self._diag_block.cpu(), self.clip_param)
