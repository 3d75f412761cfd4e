"""Distillation: rsl_rl's second algorithm on the MI355X hot path -- behaviour cloning of a trained teacher into the student of a
StudentTeacher policy, on the states the student itself visits (DAgger style).

A subclass of PPO, so the runner's loop plans, both rollout forms, the sinks, logging, save and load carry over.  The rollout is PPO's:
the student acts with its noise; the critic's values are computed as ever and then ignored.  compute_returns() runs no GAE: it makes one
pass of the teacher over the T N stored observation rows into storage.teacher_actions.  update() walks the storage in slices of
`gradient_length` steps, in storage order (rsl_rl's order: no permutation), one hgym_bc_grad + hgym_ppo_apply -- one Adam step -- per
slice and epoch.  Nothing but the student is trained: the critic and sigma keep their bits through a whole run.

Distillation.train_critic (off by default): the rollout already pays for the critic's tiles and stores rewards, dones
and values, so compute_returns() runs PPO's own returns machinery ahead of the teacher's pass and update() calls hgym_bc_vf_grad in place
of hgym_bc_grad -- the student's gradient path is the same, so the student keeps the bits of a run with the option off, and the checkpoint
leaves with a critic trained on the student's own returns.
"""
import math

import torch

from . import rnd as rnd_module
from . import smoothness as smooth_module
from .log_block import mean_of_sums
from .ppo import PPO
from .student_teacher import StudentTeacher

NO_CLIP = 3.0e38      # max_grad_norm=None: a clip that never binds (coef = min(max_norm / (norm + 1e-6), 1) = 1)


class Distillation(PPO):
    policy: StudentTeacher
    LOSS_TYPES = ("mse", "huber")
    # the critic is trained beside the student, on PPO's returns of the student's own rollouts: value_loss_coef, use_clipped_value_loss,
    # clip_param, gamma and lam are PPO's attributes of those names (PPO's defaults unless set).  Read once, in init_storage.
    train_critic = False

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 huber_delta=1.0, device="cpu"):
        if loss_type not in self.LOSS_TYPES:
            raise ValueError("Distillation.loss_type=%r: one of %s" % (loss_type, ", ".join(self.LOSS_TYPES)))
        if loss_type == "huber" and not (float(huber_delta) > 0.0 and math.isfinite(float(huber_delta))):
            raise ValueError("Distillation.huber_delta=%r: must be finite and > 0" % (huber_delta,))
        if int(gradient_length) != gradient_length or gradient_length < 1:
            raise ValueError("Distillation.gradient_length=%r: must be an integer >= 1" % (gradient_length,))
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):
            raise ValueError("Distillation.max_grad_norm=%r: must be None or > 0" % (max_grad_norm,))
        super().__init__(policy, num_learning_epochs=num_learning_epochs, num_mini_batches=1, learning_rate=learning_rate,
                         max_grad_norm=NO_CLIP if max_grad_norm is None else float(max_grad_norm), schedule="fixed", desired_kl=None,
                         device=device)
        self.policy = policy
        self.gradient_length = int(gradient_length)
        self.loss_type, self.huber_delta = loss_type, float(huber_delta)
        self.last_behavior_loss = None
        self.last_value_loss = None      # train_critic: the mean value loss per Adam step of the last update read
        self._bc_sums = self._vf_sums = None

    @staticmethod
    def check_setup(policy, num_transitions_per_env, gradient_length, world=1, symmetry=None, mirror_loss_coef=0.0,
                    advantage_normalization="batch"):
        """What init_storage refuses, as a function that needs no device (ValueError each): more than one rank; symmetry, the mirror loss or
        an advantage normalisation other than the default; a policy that is not a StudentTeacher; T % gradient_length != 0 (rsl_rl
        silently carries the remainder over to the next rollout)."""
        if int(world) > 1:
            raise ValueError("Distillation runs on one rank (world size %d)" % int(world))
        if symmetry is not None or float(mirror_loss_coef or 0.0) != 0.0:
            raise ValueError("Distillation does not support PPO.symmetry / PPO.mirror_loss_coef")
        if advantage_normalization != PPO.advantage_normalization:
            raise ValueError("Distillation uses no advantages: advantage_normalization=%r must stay %r"
                             % (advantage_normalization, PPO.advantage_normalization))
        if not isinstance(policy, StudentTeacher):
            raise ValueError("Distillation needs a StudentTeacher policy, not %s" % type(policy).__name__)
        if int(num_transitions_per_env) % int(gradient_length) != 0:
            raise ValueError("Distillation: num_steps_per_env=%d is not a multiple of gradient_length=%d"
                             % (int(num_transitions_per_env), int(gradient_length)))

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        if self.rnd is not None:
            rnd_module.check_setup(distillation=True)
        if smooth_module.parse_config(self.smoothness, self.actor_critic.num_actor_obs) is not None:
            smooth_module.check_setup(distillation=True)
        from . import guidance as guide_module
        if guide_module.parse_config(self.guidance) is not None:
            guide_module.check_setup(distillation=True)
        from . import critic_warmup as warmup_module
        if warmup_module.parse_config(self.critic_warmup_updates) > 0:
            raise ValueError("PPO.critic_warmup_updates does not support Distillation: Distillation.train_critic trains the critic beside the student")
        if self.value_normalization:      # (a follow-up at most: a cloning run computes no returns, the critic is not trained)
            raise ValueError("PPO.value_normalization does not support Distillation: a cloning run has no returns to standardise")
        self.check_setup(self.actor_critic, num_transitions_per_env, self.gradient_length, self._world, self.symmetry,
                         self.mirror_loss_coef, self.advantage_normalization)
        # one "minibatch" is one slice: gradient_length * N rows (PPO.init_storage sizes the net's max_batch from it)
        self.num_mini_batches = int(num_transitions_per_env) // self.gradient_length
        self._bc_sums = torch.zeros(2, dtype=torch.float64, device=self.device)      # (ahead of PPO's part, which ends by building the log block)
        self._train_critic = bool(self.train_critic)
        self._vf_sums = torch.zeros(2, dtype=torch.float64, device=self.device) if self._train_critic else None
        super().init_storage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape)
        hgym, st = self._hgym, self.storage
        T, N = st.num_transitions_per_env, st.num_envs
        st.teacher_actions = torch.zeros(T, N, *action_shape, dtype=torch.float32, device=self.device)
        self._bc_cfg = hgym.make_bc_config(self.loss_type, self.huber_delta)
        # the step is hgym_ppo_apply's: no learning-rate rule, its own norm pass, the clip as asked for
        self._ppo_cfg = hgym.make_ppo_config(max_grad_norm=self.max_grad_norm, desired_kl=0.0, adaptive=False, world_size=1,
                                             grad_norm_ready=False)
        self._rows = torch.arange(T * N, dtype=torch.int64, device=self.device)
        if self._train_critic:      # (make_vf_config refuses a clip range or a coefficient that is negative or not finite: ValueError)
            self._vf_cfg = hgym.make_vf_config(self.clip_param, self.value_loss_coef, clipped_value_loss=bool(self.use_clipped_value_loss))

    # ------------------------------------------------------------------
    def compute_returns(self, last_critic_obs):
        """No returns: the teacher's mean action for every stored observation row -> storage.teacher_actions, one pass in pieces of at
        most max_batch rows.  Nothing inside a rollout consumes the teacher's action, so the pass is deferred to here, as the critic's is
        on the deferred-values path."""
        st = self.storage
        T = st.num_transitions_per_env
        if self._train_critic:
            # PPO's own returns first: the deferred critic where the rollout left it, the time-out bootstrap, GAE (the advantages are a
            # by-product nobody reads)
            PPO.compute_returns(self, last_critic_obs)
        self.actor_critic.teacher_pass(st._obs_all[:T].flatten(0, 1), st.teacher_actions.flatten(0, 1))
        self._returns_done()

    def update_capturable(self):
        return False      # the update is issued eagerly; capturing it is not built

    def _update_done(self):      # no permutation was drawn: the draw counters stay where they are
        self.storage.cleared()

    def update(self, sync=True):
        """For each epoch and each of the T / gradient_length slices in storage order: hgym_bc_grad on rows [t0 N, (t0 + gradient_length) N)
        against storage.teacher_actions, then hgym_ppo_apply.  Returns (0.0, mean_behavior_loss); sync=False: (None, None), nothing read back."""
        if not self.actor_critic.loaded_teacher:
            raise RuntimeError("teacher not loaded")
        hgym, net, st = self._hgym, self.net, self.storage
        T, N = st.num_transitions_per_env, st.num_envs
        mb = self.gradient_length * N
        obs, target = st._obs_all[:T].flatten(0, 1), st.teacher_actions.flatten(0, 1)
        sh = st.shadows()
        self._bc_sums[0:2] = 0.0
        critic = self._train_critic
        if critic:
            self._vf_sums[0:2] = 0.0
            cols = st.batch_columns()      # (obs, priv, ., values, ., returns, ...): the T N stored rows
            assert cols[0].data_ptr() == obs.data_ptr()
        for _ in range(self.num_learning_epochs):
            for k in range(T // self.gradient_length):
                rows = self._rows[k * mb:(k + 1) * mb]
                if critic:      # the student's regression and the critic's value loss in one call: bc_grad, then vf_grad beside it, bit for bit
                    batch = hgym.make_vf_batch(cols[1], cols[3], cols[5], rows, priv_bf16=None if sh is None else sh[1], obs=obs,
                                               obs_bf16=None if sh is None else sh[0])
                    net.bc_vf_grad(self._bc_cfg, self._vf_cfg, batch, target, self._bc_sums, self._vf_sums)
                else:
                    batch = hgym.make_bc_batch(obs, rows, None if sh is None else sh[0])
                    net.bc_grad(self._bc_cfg, batch, target, self._bc_sums)
                net.ppo_apply(self._ppo_cfg)
        st.rotate()
        self._update_done()
        if not sync:
            return None, None
        self.read_log(self.log_block().cpu())
        return (self.last_value_loss if critic else 0.0), self.last_behavior_loss

    def _log_parts(self):
        """opt | bc(2) | vf(2): opt_state and, behind it, the behaviour loss's two sums, then -- train_critic -- the value loss's two (every
        option of PPO's block is refused here)."""
        vf = getattr(self, "_vf_sums", None)
        return [("opt", self.net.opt_state), ("bc", self._bc_sums)] + ([] if vf is None else [("vf", vf)])

    def read_log(self, block):      # PPO's, and last_behavior_loss, last_value_loss; log_scalars: Loss/behavior behind PPO's pairs
        self.last_behavior_loss = self.behavior_loss_from(block)
        o = super().read_log(block)
        parts = self._log.split(block)
        if "vf" in parts:      # train_critic: Loss/value_function is the critic's mean value loss per Adam step
            self.last_value_loss = mean_of_sums(parts["vf"])
            o = dict(o, mean_value_loss=self.last_value_loss)
        return o

    def log_scalars(self):
        return super().log_scalars() + ([] if self.last_behavior_loss is None else [("Loss/behavior", self.last_behavior_loss)])

    def behavior_loss_from(self, block):
        """The mean behaviour loss per Adam step of the last update from a host copy of log_block()."""
        return mean_of_sums(self._log.split(block)["bc"])

    # ------------------------------------------------------------------ what a cloning run has no use for
    def diagnostics_prepare(self):
        raise RuntimeError("Distillation has no PPO diagnostics (no ratios, no advantages, no trained critic)")

    def diagnostics(self, sync=True):
        raise RuntimeError("Distillation has no PPO diagnostics (no ratios, no advantages, no trained critic)")
