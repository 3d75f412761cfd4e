"""OnPolicyRunner with the reference's interface (algo/ppo/on_policy_runner.py:45-307): rollout / learn loop,
checkpoint save / load (same dict keys), inference-policy getters, console + optional TensorBoard logging.

The env writes its observations straight into the rollout-storage slots, and episode book-keeping stays on the device,
read back once per iteration (the reference syncs the host every step, :146-152)."""
import gc
import os
import statistics
import time
from collections import deque
from dataclasses import dataclass
from datetime import datetime
from typing import Optional

import torch

from . import checkpoint as ckpt
from .checkpoint import NORM_KEYS, RND_STATE_KEY, _check_norm_keys  # noqa: F401  (re-exported: tests and tools read them here)
from .ppo import PPO
from .actor_critic import ActorCritic
from .student_teacher import StudentTeacher  # noqa: F401  (policy_class_name is eval'ed below)
from .distillation import Distillation  # noqa: F401  (algorithm_class_name likewise)
from humanoid.algo.vec_env import VecEnv

try:  # optional: logging back-ends are not part of the hot path
    from torch.utils.tensorboard import SummaryWriter
except Exception:  # pragma: no cover
    SummaryWriter = None
try:
    import wandb
except Exception:  # pragma: no cover
    wandb = None


@dataclass(frozen=True)
class _LoopPlan:
    """How one learn() call runs its iterations (_plan_loop)."""
    zero_copy: bool         # the env writes its observations straight into the rollout storage slots (bind_outputs)
    graph: bool             # the rollout is captured into a HIP graph and replayed (HGYM_GRAPH)
    env_sink: bool          # the env's step finaliser also stores the transition's scalar columns (bind_transition, HGYM_ENV_SINK)
    log_sink: bool          # ... and keeps the logging book-keeping on the device, read once per iteration (bind_log_sink, HGYM_LOG_SINK)
    defer_fin: bool         # ... and rides in the next policy launch: nothing on the host reads the per-step extras (HGYM_DEFER_FIN)
    fuse: Optional[str]     # one launch per vec-step (HGYM_FUSE_ROLLOUT): None, "inline" or "deferred" (the critic after the rollout)
    async_mode: Optional[str]   # nothing read back inside an iteration (HGYM_ASYNC): None, "events" (no logging) or "log" (log sink)
    graph_update: bool      # compute_returns() + update() as a second HIP graph, behind async_mode only (HGYM_GRAPH_UPDATE)


def _plan_loop(env, alg, device, log_on):
    """The loop plan from the native extensions of env and alg and the HGYM_* knobs; no side effects.  Without them: the plain path."""
    knob = lambda name: os.environ.get(name, "1") != "0"
    cuda = str(device).startswith("cuda")
    st = alg.storage
    zero_copy = bool(getattr(st, "_obs_all", None) is not None and getattr(st, "_priv_all", None) is not None
                     and hasattr(env, "bind_outputs") and env.get_privileged_observations() is not None)
    graph = bool(zero_copy and cuda and knob("HGYM_GRAPH") and hasattr(torch.cuda, "CUDAGraph"))
    env_sink = bool(zero_copy and hasattr(env, "bind_transition") and hasattr(alg, "transition_sink")
                    and getattr(env.cfg.env, "send_timeouts", False) and knob("HGYM_ENV_SINK"))
    log_sink = bool(log_on and env_sink and hasattr(env, "bind_log_sink") and knob("HGYM_LOG_SINK") and env.log_sink_supported())
    defer_fin = bool(env_sink and not (log_on and not log_sink) and hasattr(env, "take_pending_finalize") and isinstance(alg, PPO)
                     and knob("HGYM_DEFER_FIN"))
    fuse = (env.rollout_fused_mode(alg.net) if (defer_fin and hasattr(env, "rollout_fused_mode") and hasattr(alg, "fused_rollout_step")
                                                and knob("HGYM_FUSE_ROLLOUT")) else None)
    fuse = "inline" if (fuse == "deferred" and not hasattr(alg, "deferred_values")) else fuse
    # PPO.value_normalization: the inline form computes V and consumes it (the time-out bootstrap) in the same launch, with no place for the
    # denormalisation between the two -- the critic runs behind the rollout instead, followed by the denormalise launches
    fuse = "deferred" if (fuse == "inline" and alg.value_normalizer is not None) else fuse
    async_ok = cuda and isinstance(alg, PPO) and knob("HGYM_ASYNC")
    async_mode = "events" if (not log_on and async_ok) else "log" if (log_sink and async_ok) else None
    graph_update = bool(graph and async_mode is not None and hasattr(alg, "update_capturable") and alg.update_capturable()
                        and knob("HGYM_GRAPH_UPDATE"))
    return _LoopPlan(zero_copy, graph, env_sink, log_sink, defer_fin, fuse, async_mode, graph_update)


class _CapturedGraph:
    """Launches learn() repeats every iteration, as one HIP graph.  run(): the first call runs eager() (and marks warm), the next captures
    capture() and replays it once, later ones with the same key replay and call after_replay(held), held = what capture() returned."""

    def __init__(self):
        self.graph, self.key, self.held, self.warm = None, None, None, False

    def valid(self, key):
        return self.graph is not None and self.key == key

    def run(self, on, key, eager, capture, after_replay):
        if on and self.valid(key):
            self.graph.replay()
            after_replay(self.held)
            return self.held
        if not (on and self.warm):
            out, self.warm = eager(), True
            return out
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        # thread-local capture mode: with torch.distributed initialised, the RCCL watchdog thread polls events concurrently.  Inference
        # mode: capture_begin updates the generator's graph-state tensors in place, and the first capture created them as inference tensors
        # No garbage collection inside the capture: a collection that starts while the stream is capturing runs, on the capturing thread, the
        # finalisers of whatever cyclic garbage the process has accumulated -- runners, nets and captured graphs of earlier learn() calls --
        # and releasing device objects is not an operation a capture permits (seen as an abort of the process with the interpreter in
        # "Garbage-collecting" under this frame).  torch.cuda.graph collects once itself before the capture begins.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.inference_mode(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                held = capture()
        finally:
            if gc_was_on:
                gc.enable()
        self.graph, self.key, self.held = graph, key, held
        graph.replay()
        return held


class _EpisodeLog:
    """Host logging book-keeping (on: no log sink): per-step extras["episode"], running return / length per env, and the reference's
    rewbuffer / lenbuffer -- deque(maxlen=100) -- as two circular buffers in device tensors: ring (2, 101) fp32 (slot 100 takes the
    writes of the envs that did not finish), meta = [head, fill] int64.  Every operation is stream-ordered torch with fixed shapes, so the
    loop needs no read-back per step and can be captured; read() is the one read-back per iteration."""
    RING = 100

    def __init__(self, on, tensors):
        self.on, self.ep_infos = on, []
        self.reward_sum, self.length, self.ring, self.meta = tensors

    @classmethod
    def tensors(cls, num_envs, device):
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
        return [z(num_envs), z(num_envs), z(2, cls.RING + 1), z(2, dtype=torch.int64)]

    def step(self, rewards, dones):
        """on_policy_runner.py:144-154: cur_reward_sum += rewards, cur_episode_length += 1, the buffers .extend(cur[new_ids]) in
        ascending env order, cur[new_ids] = 0.  The k-th finished env of the step goes to slot (head + k) % 100; of more than 100 only
        the last 100 are written (what the deque keeps), so no slot is written twice."""
        R = self.RING
        self.reward_sum.add_(rewards.reshape(-1))
        self.length.add_(1)
        d = dones.reshape(-1) > 0
        incl = torch.cumsum(d, 0)
        total = incl[-1]
        order = incl - 1
        keep = d & (order >= total - R)
        head, fill = self.meta[0].clone(), self.meta[1].clone()
        pos = torch.where(keep, (head + order) % R, torch.full_like(order, R))
        self.ring[0].scatter_(0, pos, self.reward_sum)
        self.ring[1].scatter_(0, pos, self.length)
        self.meta[0] = (head + total) % R
        self.meta[1] = torch.clamp(fill + total, max=R)
        self.reward_sum.masked_fill_(d, 0.0)
        self.length.masked_fill_(d, 0.0)

    def read(self):
        """(rewbuffer, lenbuffer) as deques, oldest episode first."""
        ring, (head, fill) = self.ring.cpu(), self.meta.cpu().tolist()
        slots = [(head - fill + k) % self.RING for k in range(fill)]
        return tuple(deque((float(ring[j, s]) for s in slots), maxlen=self.RING) for j in (0, 1))


SYMMETRY_KEYS = ("mirror_loss_coef", "symmetry_augmentation", "symmetry_cfg")      # native keys beside `symmetry`; none is a parameter of PPO.__init__


def _split_algorithm_cfg(alg_cfg):
    """The train config's algorithm block -> (keyword arguments of PPO.__init__, symmetry on?).  `symmetry` is a native key (absent:
    off), not a parameter of the reference's PPO: it is taken out here and becomes PPO.symmetry.  The mirror loss's keys (SYMMETRY_KEYS)
    are taken out as well; _split_symmetry_cfg reads them.  So are the advantage normalisation's (ADVANTAGE_KEYS; _split_advantage_cfg)."""
    kwargs = dict(alg_cfg)
    for k in SYMMETRY_KEYS + ADVANTAGE_KEYS + VALUE_NORM_KEYS + (RND_KEY, SMOOTH_KEY, GUIDE_KEY, WARMUP_KEY, TRAIN_CRITIC_KEY, NOISE_KEY):
        kwargs.pop(k, None)
    return kwargs, bool(kwargs.pop("symmetry", False))


ADVANTAGE_KEYS = ("advantage_normalization", "normalize_advantage_per_mini_batch")      # neither is a parameter of PPO.__init__
SMOOTH_KEY = "smoothness_cfg"      # the smoothness regulariser's block (humanoid.algo.ppo.smoothness.parse_config); absent or None: off
VALUE_NORM_KEYS = ("value_normalization", "value_normalization_eps")      # PPO.value_normalization / _eps; neither is a parameter of PPO.__init__
GUIDE_KEY = "guidance_cfg"      # guidance by a frozen teacher (humanoid.algo.ppo.guidance.parse_config); absent or None: off
WARMUP_KEY = "critic_warmup_updates"      # PPO.critic_warmup_updates: the first n updates move the critic alone; absent or 0: off
TRAIN_CRITIC_KEY = "train_critic"      # Distillation.train_critic: a cloning run also trains the critic; absent: off
# with it, PPO's own value-loss and returns settings from the same block: not parameters of Distillation.__init__, set as attributes
DISTILL_CRITIC_KEYS = ("value_loss_coef", "use_clipped_value_loss", "clip_param", "gamma", "lam")
NOISE_KEY = "exploration_noise_cfg"      # temporally correlated exploration noise (humanoid.algo.ppo.exploration_noise.parse_config); absent or None: off
RND_KEY = "rnd_cfg"      # rsl_rl's Random Network Distillation block (humanoid.algo.ppo.rnd.parse_config); absent or None: off


def _split_advantage_cfg(alg_cfg):
    """The train config's algorithm block -> PPO.advantage_normalization: "batch" (the default), "minibatch" or "none".  Native key:
    `advantage_normalization`.  rsl_rl's `normalize_advantage_per_mini_batch` is accepted too: True is "minibatch", False is "batch"; set
    beside a native key that says otherwise: ValueError, as is an unknown mode.  The caller's dict is left alone."""
    modes = PPO.ADVANTAGE_NORMALIZATIONS
    mode = alg_cfg.get("advantage_normalization")
    if mode is not None and mode not in modes:
        raise ValueError("algorithm.advantage_normalization=%r: one of %s" % (mode, ", ".join(modes)))
    if alg_cfg.get("normalize_advantage_per_mini_batch") is not None:
        theirs = "minibatch" if bool(alg_cfg["normalize_advantage_per_mini_batch"]) else "batch"
        if mode is not None and mode != theirs:
            raise ValueError("algorithm.normalize_advantage_per_mini_batch=%r disagrees with algorithm.advantage_normalization=%r"
                             % (alg_cfg["normalize_advantage_per_mini_batch"], mode))
        mode = theirs
    return "batch" if mode is None else mode


def _split_symmetry_cfg(alg_cfg):
    """The train config's algorithm block -> (augmentation on?, mirror_loss_coef).  Native keys: `symmetry` (augmentation, as ever),
    `symmetry_augmentation` (default True; False with `symmetry` keeps the tables but not the augmentation) and `mirror_loss_coef`
    (default 0: off).  rsl_rl's spelling is accepted too: `symmetry_cfg = {use_data_augmentation, use_mirror_loss, mirror_loss_coeff}`;
    a native key and its rsl_rl twin that disagree: ValueError.  The caller's dict is left alone."""
    augmentation = bool(alg_cfg.get("symmetry", False)) and bool(alg_cfg.get("symmetry_augmentation", True))
    coef = float(alg_cfg.get("mirror_loss_coef", 0.0) or 0.0)
    sc = alg_cfg.get("symmetry_cfg")
    if sc:
        sc = dict(sc)
        unknown = set(sc) - {"use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff"}
        if unknown:
            raise ValueError("algorithm.symmetry_cfg: unknown keys %s (use_data_augmentation, use_mirror_loss, mirror_loss_coeff)" % sorted(unknown))
        if "use_data_augmentation" in sc:
            aug = bool(sc["use_data_augmentation"])
            if ("symmetry" in alg_cfg or "symmetry_augmentation" in alg_cfg) and aug != augmentation:
                raise ValueError("algorithm.symmetry_cfg.use_data_augmentation=%r disagrees with algorithm.symmetry / symmetry_augmentation" % (aug,))
            augmentation = aug
        c = float(sc.get("mirror_loss_coeff", 0.0) or 0.0) if sc.get("use_mirror_loss", False) else 0.0
        if "use_mirror_loss" in sc or "mirror_loss_coeff" in sc:
            if "mirror_loss_coef" in alg_cfg and c != coef:
                raise ValueError("algorithm.symmetry_cfg's mirror loss (%r) disagrees with algorithm.mirror_loss_coef=%r" % (c, coef))
            coef = c
    return augmentation, coef


def _split_policy_cfg(policy_cfg, runner_cfg):
    """The keyword arguments of ActorCritic from the train config's policy block.  `empirical_normalization` is read from the policy
    block or -- rsl_rl's place for it -- from the runner block and passed on; set in both, the two must agree (ValueError)."""
    kwargs = dict(policy_cfg)
    if "empirical_normalization" in runner_cfg:
        r = bool(runner_cfg["empirical_normalization"])
        if "empirical_normalization" in kwargs and bool(kwargs["empirical_normalization"]) != r:
            raise ValueError("empirical_normalization is %r in the policy block and %r in the runner block of the train config"
                             % (kwargs["empirical_normalization"], runner_cfg["empirical_normalization"]))
        kwargs["empirical_normalization"] = r
    return kwargs


class OnPolicyRunner:
    def __init__(self, env: VecEnv, train_cfg, log_dir=None, device="cpu"):
        self.cfg = train_cfg["runner"]
        self.alg_cfg = train_cfg["algorithm"]
        self.policy_cfg = train_cfg["policy"]
        self.all_cfg = train_cfg
        self.wandb_run_name = (datetime.now().strftime("%b%d_%H-%M-%S") + "_" + train_cfg["runner"]["experiment_name"] + "_"
                               + train_cfg["runner"]["run_name"])
        self.device = device
        self.env = env
        num_critic_obs = self.env.num_privileged_obs if self.env.num_privileged_obs is not None else self.env.num_obs
        actor_critic_class = eval(self.cfg["policy_class_name"])  # ActorCritic
        actor_critic = actor_critic_class(self.env.num_obs, num_critic_obs, self.env.num_actions,
                                          **_split_policy_cfg(self.policy_cfg, self.cfg)).to(self.device)
        alg_class = eval(self.cfg["algorithm_class_name"])  # PPO
        alg_kwargs, symmetry = _split_algorithm_cfg(self.alg_cfg)
        augmentation, mirror_loss_coef = _split_symmetry_cfg(self.alg_cfg)
        distill_critic = {k: alg_kwargs.pop(k) for k in DISTILL_CRITIC_KEYS if k in alg_kwargs} if issubclass(alg_class, Distillation) else {}
        self.alg = alg_class(actor_critic, device=self.device, **alg_kwargs)
        for k, v in distill_critic.items():      # Distillation.train_critic's value loss and returns; read by init_storage / compute_returns
            setattr(self.alg, k, v)
        if self.alg_cfg.get(TRAIN_CRITIC_KEY) is not None:      # read by init_storage below
            if not issubclass(alg_class, Distillation):
                raise ValueError("algorithm.train_critic is Distillation's option; %s trains its critic anyway" % alg_class.__name__)
            self.alg.train_critic = bool(self.alg_cfg[TRAIN_CRITIC_KEY])
        if self.alg_cfg.get(WARMUP_KEY) is not None:      # critic-only warm-up; read by init_storage below
            self.alg.critic_warmup_updates = self.alg_cfg[WARMUP_KEY]
        if symmetry or augmentation or mirror_loss_coef > 0.0:        # left-right symmetry with XBot-L's tables; read by init_storage below
            from humanoid.utils.symmetry import xbot_l_mirror
            self.alg.symmetry = xbot_l_mirror(self.env.cfg)
            self.alg.symmetry_augmentation = augmentation
            self.alg.mirror_loss_coef = mirror_loss_coef
        if any(self.alg_cfg.get(k) is not None for k in ADVANTAGE_KEYS):      # read by init_storage below
            self.alg.advantage_normalization = _split_advantage_cfg(self.alg_cfg)
        if self.alg_cfg.get(RND_KEY) is not None:      # Random Network Distillation; read by init_storage below
            from .rnd import RandomNetworkDistillation
            env_cfg = getattr(getattr(self.env, "cfg", None), "env", None)
            self.alg.rnd = RandomNetworkDistillation(self.env.num_obs, num_critic_obs, self.alg_cfg[RND_KEY],
                                                     critic_frame=getattr(env_cfg, "single_num_privileged_obs", None),
                                                     activation=getattr(actor_critic, "activation", None))
        if self.alg_cfg.get(SMOOTH_KEY) is not None:      # the smoothness regulariser; read by init_storage below
            from . import smoothness as smooth_module
            sc = dict(self.alg_cfg[SMOOTH_KEY])
            if sc.get("noise_std") is None:      # the sensor noise the env itself models, per stacked column
                sc["noise_std"] = smooth_module.env_noise_std(getattr(self.env, "cfg", None), getattr(self.env, "noise_scale_vec", None),
                                                              self.env.num_obs)
            self.alg.smoothness = sc
        if self.alg_cfg.get(GUIDE_KEY) is not None:      # guidance by a frozen teacher; read by init_storage below
            self.alg.guidance = dict(self.alg_cfg[GUIDE_KEY])
        if self.alg_cfg.get(NOISE_KEY) is not None:      # temporally correlated exploration noise; read by init_storage below
            self.alg.exploration_noise = dict(self.alg_cfg[NOISE_KEY])
        if self.alg_cfg.get("value_normalization") is not None:      # value targets standardised by running statistics; read by init_storage below
            self.alg.value_normalization = bool(self.alg_cfg["value_normalization"])
        if self.alg_cfg.get("value_normalization_eps") is not None:
            self.alg.value_normalization_eps = float(self.alg_cfg["value_normalization_eps"])
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]
        self.alg.init_storage(self.env.num_envs, self.num_steps_per_env, [self.env.num_obs], [self.env.num_privileged_obs],
                              [self.env.num_actions])
        self.log_dir = log_dir
        self.writer = None
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.last_collection_time = self.last_learn_time = 0.0
        self._rollout_capture = _CapturedGraph()     # the rollout as a HIP graph, and the tensors it owns
        self._update_capture = _CapturedGraph()      # compute_returns() + update() as a second HIP graph
        self._eval_capture = _CapturedGraph()        # the fused evaluation rollout as a HIP graph of its own (evaluate)
        self.eval_env = None                         # set_eval_env: learn() evaluates on it every cfg["eval_interval"] iterations
        self.last_eval = None
        self.last_diag = None                        # PPO.diagnostics() of the last iteration cfg["diag_interval"] selected (learn)
        self.last_diag_iteration = None
        self._diag_pin = None
        self._keep_episode_lengths = False           # set by an exact resume (load): the next learn() keeps the restored episode lengths
        self._warned_env_state = False
        _, _ = self.env.reset()

    _graph = property(lambda self: self._rollout_capture.graph)
    _update_graph = property(lambda self: self._update_capture.graph)

    # ------------------------------------------------------------------
    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        if getattr(self.alg.actor_critic, "loaded_teacher", True) is False:      # a StudentTeacher that was never given its teacher (load)
            raise RuntimeError("teacher not loaded")
        self._open_writer()
        if init_at_random_ep_len and self._keep_episode_lengths:
            init_at_random_ep_len = False            # (once: the episode lengths are part of the env state load() has just restored)
        self._keep_episode_lengths = False
        exact = ckpt.exact_resume_on(self.cfg, getattr(self.alg, "_world", 1), self)
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf, high=int(self.env.max_episode_length))
        env, alg, log_on = self.env, self.alg, self.log_dir is not None
        plan = _plan_loop(env, alg, self.device, log_on)
        obs, privileged_obs = env.get_observations(), env.get_privileged_observations()
        obs, critic_obs = obs.to(self.device), (privileged_obs if privileged_obs is not None else obs).to(self.device)
        obs_all, priv_all = getattr(alg.storage, "_obs_all", None), getattr(alg.storage, "_priv_all", None)
        if plan.zero_copy:
            obs_all[0].copy_(obs)
            priv_all[0].copy_(critic_obs)
            obs, critic_obs = obs_all[0], priv_all[0]
        alg.actor_critic.train()
        log = _EpisodeLog(log_on and not plan.log_sink, _EpisodeLog.tensors(env.num_envs, self.device))
        if plan.env_sink:
            alg.env_stores_transitions = True
        if plan.log_sink:
            env.bind_log_sink(True)
        # the captured launches hold HgymEnvConfig and the sink's gamma BY VALUE: a change between learn() calls (what a curriculum
        # script does) must re-capture, as the eager reference would simply see it
        gkey = (id(env), alg.rollout_graph_key(), log_on, plan.log_sink, plan.env_sink, plan.defer_fin, plan.fuse,
                env.rollout_graph_key() if hasattr(env, "rollout_graph_key") else None)
        ukey = (gkey, alg.update_graph_key(), plan.fuse == "deferred") if plan.graph_update else None
        if not plan.graph_update:
            self._update_capture.graph = None
        pending, marks = None, []
        # cfg["diag_interval"] (0 / absent: never): every that many iterations PPO.diagnostics() right behind the update, outside both graphs
        diag_every = int(self.cfg.get("diag_interval", 0) or 0) if hasattr(alg, "diagnostics") else 0
        diag_wait = None
        try:
            for it in range(self.current_learning_iteration, self.current_learning_iteration + num_learning_iterations):
                start = time.time()
                if plan.async_mode:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()
                with torch.inference_mode():
                    obs, critic_obs, log = self._collect(plan, gkey, obs, critic_obs, log)
                    if plan.async_mode:
                        ev[1].record()
                    elif str(self.device).startswith("cuda"):
                        torch.cuda.synchronize()
                stop = time.time()
                collection_time, start = stop - start, stop
                diag_now = diag_every > 0 and (it + 1) % diag_every == 0
                if diag_now:
                    alg.diagnostics_prepare()       # slot 0's observation rows, before the update's clear() rotates them away
                if plan.graph_update and (getattr(alg, "_guide", None) is not None or getattr(alg, "_warmup", None) is not None):
                    # the options whose graph key changes inside a run: when guidance's schedule runs out, or the last critic-only update
                    # is done, the update is the plain one again
                    if alg._guide is not None:
                        alg._guide.retire_if_run_out()
                    if alg._warmup is not None:
                        alg._warmup.retire_if_done()
                    ukey = (gkey, alg.update_graph_key(), plan.fuse == "deferred")
                mean_value_loss, mean_surrogate_loss = self._learn_step(plan, gkey, ukey, critic_obs, obs)
                diag = alg.diagnostics(sync=False) if diag_now else None       # enqueued; read where this path reads anything
                if plan.zero_copy:                  # storage.clear() rotated slot T into slot 0
                    obs, critic_obs = obs_all[0], priv_all[0]
                if it % self.save_interval == 0:
                    self._check_replicas("iteration %d" % it)       # (data-parallel runs only; collective: every rank, same iteration)
                learn_time = time.time() - start
                if plan.async_mode:
                    ev[2].record()
                if plan.async_mode == "events":
                    marks.append(ev)
                    if diag is not None:
                        diag_wait = (it, self._diag_snapshot(diag, 0))      # read once, behind the loop's last event
                elif plan.async_mode == "log":
                    pending = self._finish_async_log(it, ev, pending, num_learning_iterations, diag)
                else:
                    if diag is not None:
                        self._diag_publish(it, diag.cpu())      # (this path synchronises every iteration anyway)
                    self._finish_sync(plan, log, dict(it=it, num_learning_iterations=num_learning_iterations,
                                                      collection_time=collection_time, learn_time=learn_time,
                                                      mean_value_loss=mean_value_loss, mean_surrogate_loss=mean_surrogate_loss))
                if log_on and it % self.save_interval == 0:
                    # (current_learning_iteration still holds the value from the start of learn(), the reference's quirk, and "iter"
                    # in model_<it>.pt keeps it; the sidecar records the true count)
                    self.save(os.path.join(self.log_dir, "model_{}.pt".format(it)), wait=False, env_state=exact, iterations_done=it + 1)
                self._maybe_evaluate(it)            # behind the iteration's timing marks, like everything that is not the iteration
        finally:
            # also on an exception inside the loop: the last finished iteration's log block is printed, the env's bindings released
            if pending is not None:
                try:
                    self._log_flush(pending, num_learning_iterations)
                except Exception:      # the device may be the thing that failed
                    pass
            self._unbind(plan)
        if marks:
            self._read_event_times(marks)
        if diag_wait is not None:
            torch.cuda.synchronize()
            self._diag_publish(diag_wait[0], diag_wait[1])
        self.current_learning_iteration += num_learning_iterations
        self._check_replicas("end of learn() at iteration %d" % self.current_learning_iteration)
        if log_on:      # (the background writer finishes the file; wait_for_saves() / load() / interpreter exit wait for it: save())
            self.save(os.path.join(self.log_dir, "model_{}.pt".format(self.current_learning_iteration)), wait=False, env_state=exact)

    # ------------------------------------------------------------------ evaluation on mean actions
    def set_eval_env(self, env):
        """The env learn() evaluates on every cfg["eval_interval"] iterations (0 / absent: never) for cfg["eval_steps"] steps: a
        LeggedRobot of its own, never the training env."""
        if env is self.env:
            raise ValueError("the evaluation env must not be the training env")
        self.eval_env = env

    def _maybe_evaluate(self, it):
        every = int(self.cfg.get("eval_interval", 0) or 0)
        if every <= 0 or self.eval_env is None or (it + 1) % every != 0:
            return
        from . import dist_utils
        if dist_utils.active() and torch.distributed.get_rank() != 0:       # N > 1 ranks: rank 0 evaluates (no collective inside)
            return
        self.last_eval = self.evaluate(self.eval_env, int(self.cfg.get("eval_steps", self.num_steps_per_env)))
        if self.writer is not None:
            for k, v in self.last_eval.items():
                self.writer.add_scalar("Eval/" + k, v, it)

    def evaluate(self, env, num_steps, reset=True, fused=None):
        """How good is the current policy: num_steps vec-steps of `env` on the policy's MEAN action (what play.py and an exported policy
        run), summarised over all its envs.  env: a separate LeggedRobot -- any num_envs, its own config (play.py's overrides are the
        typical ones) -- never the training env.  reset: env.reset() first; without it the running episodes are counted from here.

        Where env.eval_rollout_supported(net) (and fused is not False) every vec-step is ONE launch (hgym_rollout_eval_step: actor tile
        with action = mu + env step + the previous step's finaliser) and the whole evaluation one replayed HIP graph; otherwise the
        policy's mean (act_inference) + env.step per step (other activations, widths, fp32, terrain options, user-defined reward terms).
        Both paths feed the same device-side accumulator (hgym_eval_accumulate: fp64 sums in a fixed order), read back once, so the
        result does not depend on the path.

        Returns python floats: episodes (int), mean_episode_return, mean_episode_length, timeout_fraction, fall_fraction (over the
        episodes that ended inside the evaluation), mean_reward_per_step, lin_vel_tracking_error, ang_vel_tracking_error (over all
        env-steps) and rew_<term> for the kernel's reward terms (mean episode sum / episode_length_s, as extras["episode"] divides;
        the terms of an episode's last step are not in them: the env step consumes the sums inside its launch).  With zero finished
        episodes the episode fields and rew_<term> are nan and `episodes` is 0.

        No side effect on training: the rollout storage, the policy's sampling step (PPO._sample_step), the permutation draw number,
        the training env and the two captured training graphs are not touched."""
        if env is self.env:
            raise ValueError("evaluate() needs an env of its own: the training env's state belongs to learn()")
        num_steps = int(num_steps)
        if num_steps <= 0:
            raise ValueError("num_steps=%d" % num_steps)
        ac, net = self.alg.actor_critic, getattr(self.alg, "net", None)
        use_fused = bool(fused is not False and net is not None and hasattr(env, "eval_rollout_supported") and env.eval_rollout_supported(net))
        if fused is True and not use_fused:
            raise RuntimeError("fused=True, but env.eval_rollout_supported(net) is False for this env / policy")
        with torch.inference_mode():
            if reset:
                env.reset()
            env.eval_prepare(keep_episodes=not reset)
            if use_fused:
                def launches():
                    env.eval_reset()
                    env.eval_begin(net, num_steps)
                    for i in range(num_steps):
                        env.eval_step(i)
                    env.eval_end()
                    return env, net

                graph_on = (str(self.device).startswith("cuda") and os.environ.get("HGYM_GRAPH", "1") != "0" and hasattr(torch.cuda, "CUDAGraph"))
                # The captured launches carry the env's and the net's device addresses.  The capture HOLDS both objects (what launches()
                # returns stays in _CapturedGraph.held), so their buffers live as long as the graph does and their id()s cannot be handed
                # to other objects; a graph captured for another env or net is dropped here, never replayed.
                cap = self._eval_capture
                if cap.graph is not None and (cap.held[0] is not env or cap.held[1] is not net):
                    cap = self._eval_capture = _CapturedGraph()      # (eager now, captured at this env's next evaluation)
                key = (num_steps, env.rollout_graph_key())
                cap.run(graph_on, key, launches, launches, lambda held: None)
                env.eval_finish(num_steps)
            else:
                env.eval_reset()
                obs = env.get_observations()
                mb = int(net.cfg.max_batch) if (net is not None and obs.is_cuda) else obs.shape[0]
                for _ in range(num_steps):
                    # (an env larger than the net's max_batch: the rows in pieces)
                    a = ac.act_inference(obs) if obs.shape[0] <= mb else torch.cat([ac.act_inference(obs[k:k + mb]) for k in range(0, obs.shape[0], mb)])
                    obs = env.step(a)[0]
                    env.eval_accumulate()
            return env.eval_read()

    def _open_writer(self):
        if self.log_dir is not None and self.writer is None:
            if wandb is not None and hasattr(wandb, "init"):
                try:
                    wandb.init(project="XBot", sync_tensorboard=True, name=self.wandb_run_name, config=self.all_cfg)
                except Exception:
                    pass
            if SummaryWriter is not None:
                self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
            os.makedirs(self.log_dir, exist_ok=True)

    def _unbind(self, plan):
        if plan.zero_copy:
            self.env.bind_outputs(None, None)
        if plan.env_sink:
            self.env.bind_transition(None)
            self.alg.env_stores_transitions = False
        if plan.log_sink:
            self.env.bind_log_sink(False)

    def _collect(self, plan, gkey, obs, critic_obs, log):
        """One rollout -> (obs, critic_obs, log) after its last step.  Its few hundred launches touch fixed addresses only (storage slots,
        device-side counters): after one eager iteration they are captured into a HIP graph and replayed as one launch (plan.graph)."""
        st = self.alg.storage

        def rollout(obs, critic_obs, log):
            return self._rollout_fused(plan) if plan.fuse else self._rollout_stepwise(plan, obs, critic_obs, log)

        def capture():
            log_c = _EpisodeLog(log.on, (log.reward_sum, log.length, log.ring, log.meta))       # (the capture refills its own list at every replay)
            return dict(out=rollout(st._obs_all[0], st._priv_all[0], log_c), log=log_c, end=self.alg.rollout_end_state())

        r = self._rollout_capture.run(plan.graph, gkey, lambda: dict(out=rollout(obs, critic_obs, log), log=log), capture,
                                      lambda held: self.alg.after_rollout_replay(held["end"]))
        return r["out"] + (r["log"],)

    def _rollout_fused(self, plan):
        """act, env.step and process_env_step as ONE launch per vec-step, from the storage's slot 0.  "deferred": no critic tiles; the
        critic runs once over the stored rows behind the last step (only the time-out bootstrap needs V(s_t), and compute_returns
        applies it: ppo.py:107-108)."""
        alg, deferred = self.alg, plan.fuse == "deferred"
        alg.fused_rollout_step(self.env, self.num_steps_per_env, deferred)
        if deferred:
            alg.deferred_values()       # part of the collection (and of the captured graph): V of all T + 1 slots in one pass
        return alg.storage._obs_all[self.num_steps_per_env], alg.storage._priv_all[self.num_steps_per_env]

    def _rollout_stepwise(self, plan, obs, critic_obs, log):
        env, alg, fin = self.env, self.alg, None
        obs_all, priv_all = getattr(alg.storage, "_obs_all", None), getattr(alg.storage, "_priv_all", None)
        for i in range(self.num_steps_per_env):
            actions = alg.act(obs, critic_obs, env_fin=fin) if plan.defer_fin else alg.act(obs, critic_obs)
            if plan.zero_copy:
                env.bind_outputs(obs_all[i + 1], priv_all[i + 1])
            if plan.env_sink:
                env.bind_transition(alg.transition_sink(), defer_finalize=True) if plan.defer_fin else env.bind_transition(alg.transition_sink())
            obs, privileged_obs, rewards, dones, infos = env.step(actions)
            if plan.defer_fin:
                fin = env.take_pending_finalize()
            critic_obs = privileged_obs if privileged_obs is not None else obs
            alg.process_env_step(rewards, dones, infos, **({"stored": True} if plan.env_sink else {}))
            if log.on:
                if "episode" in infos:
                    log.ep_infos.append({k: v.clone() for k, v in infos["episode"].items()})
                log.step(rewards, dones)
        if plan.defer_fin:
            env.run_finalize(fin)           # the last step has no following policy launch
        return obs, critic_obs

    def _learn_step(self, plan, gkey, ukey, critic_obs, obs=None):
        """compute_returns() + update() -> (mean_value_loss, mean_surrogate_loss), None where not read back (PPO.update_capturable)."""
        def launches(sync=False):
            with torch.inference_mode():
                if self.alg._rnd is not None or self.alg._smooth is not None:      # (RND and the smoothness term read the state behind the last transition)
                    self.alg.compute_returns(critic_obs, last_obs=obs)
                else:
                    self.alg.compute_returns(critic_obs)
            return self.alg.update(sync=sync)

        return self._update_capture.run(plan.graph_update and self._rollout_capture.valid(gkey), ukey, lambda: launches(not plan.async_mode),
                                        launches, lambda held: self.alg.after_update_replay())

    def _diag_snapshot(self, block, slot):
        """Stream-ordered device -> pinned-host copy of a diagnostics block's sums (no host wait) -> the pinned tensor."""
        from hgym import _lib as L
        if self._diag_pin is None:
            self._diag_pin = [torch.zeros(L.DIAG_SUMS, dtype=torch.float64).pin_memory() for _ in range(2)]
        self._diag_pin[slot].copy_(block[:L.DIAG_SUMS], non_blocking=True)
        return self._diag_pin[slot]

    def _diag_publish(self, it, sums):
        """last_diag <- the dict of a host copy of the sums; Diag/<key> to the writer."""
        from hgym import diag_from_block
        self.last_diag, self.last_diag_iteration = diag_from_block(sums, getattr(self.alg, "clip_param", None)), it
        if self.writer is not None:
            for k, v in self.last_diag.items():
                self.writer.add_scalar("Diag/" + k, v, it)

    def _finish_async_log(self, it, ev, pending, num_learning_iterations, diag=None):
        """Log sink: iteration k's block is printed from pinned-host copies while the device runs k + 1.  -> the new pending block."""
        diag_pin = None if diag is None else self._diag_snapshot(diag, it & 1)      # (in front of the snapshot's event)
        snap = self._log_snapshot(self.env, self.alg, it & 1)
        snap["diag"] = diag_pin
        if pending is not None:
            self._log_flush(pending, num_learning_iterations)
        return dict(it=it, ev=ev, snap=snap)

    def _finish_sync(self, plan, log, locs):
        self.last_collection_time, self.last_learn_time = locs["collection_time"], locs["learn_time"]
        if self.log_dir is not None:
            if plan.log_sink:
                # one read-back: this iteration's mean extras["episode"] and the rings that ARE the reference's rewbuffer / lenbuffer
                ep_mean, ring_r, ring_l = self.env.log_sink_read()
                locs.update(ep_infos=[ep_mean], rewbuffer=deque(ring_r, maxlen=100), lenbuffer=deque(ring_l, maxlen=100))
            else:
                rewbuffer, lenbuffer = log.read()
                locs.update(ep_infos=log.ep_infos, rewbuffer=rewbuffer, lenbuffer=lenbuffer)
            self.log(locs)
        if self._graph is None or log is not self._rollout_capture.held["log"]:
            log.ep_infos.clear()

    def _read_event_times(self, marks):
        """Without logging the iterations' device times come from HIP events, read once here.  last_iteration_ms: iteration k's start
        event to iteration k + 1's, i.e. including whatever idles between them (bench.py reports their median)."""
        torch.cuda.synchronize()
        if hasattr(self.alg, "check_comm"):
            self.alg.check_comm()           # the asynchronous loop read nothing back: the exchange's status word, once per call
        self.last_collection_time = sum(a.elapsed_time(b) for a, b, _ in marks) * 1e-3 / len(marks)
        self.last_learn_time = sum(b.elapsed_time(c) for _, b, c in marks) * 1e-3 / len(marks)
        self.last_iteration_ms = [marks[k][0].elapsed_time(marks[k + 1][0]) for k in range(len(marks) - 1)] + [marks[-1][0].elapsed_time(marks[-1][2])]

    # ------------------------------------------------------------------
    def _check_replicas(self, what):
        """Data-parallel training: every save_interval iterations and at the end of learn() the ranks compare an exact digest of their
        parameters (and whether any rank's direct gradient exchange saw an expired wait) and ALL raise dist_utils.ReplicaMismatch if they
        differ -- a replica that silently diverged (a stale line over xGMI, a time-out only one rank noticed) would otherwise train on as
        a different policy.  No-op on one rank.  HGYM_REPLICA_CHECK=0 switches it off."""
        from . import dist_utils
        if not dist_utils.active() or os.environ.get("HGYM_REPLICA_CHECK", "1") == "0":
            return None
        alg = self.alg
        net = getattr(alg, "net", None)
        if net is None:
            return None
        expired = 0
        if alg._comm is not None and (alg._comm_p2p or alg._comm_direct_used):
            expired = int(alg._comm.read_status()[0] != 0)
        self.last_replica_digest = dist_utils.check_replicas(net.params, lr=alg.learning_rate, comm_expired=expired, what=what)
        return self.last_replica_digest

    def _log_snapshot(self, env, alg, slot):
        """Enqueue the device -> pinned-host copies of everything one iteration's log block needs (the optimiser's scalar state:
        loss sums, learning rate; the env's log sink: extras["episode"] sums and the last-100-episodes rings; the mean action
        std), then clear the sink's per-iteration sums.  Stream-ordered behind the update; read in _log_flush after the event."""
        if getattr(self, "_log_pin", None) is None:
            mk = lambda n, dt: [torch.empty(n, dtype=dt).pin_memory() for _ in range(2)]
            self._log_pin = dict(opt=mk(alg.log_block().numel(), alg.net.opt_state.dtype), ls=mk(env._buf.log_stats.numel(), torch.float32),
                                 std=mk(1, torch.float32))
        pin = self._log_pin
        pin["opt"][slot].copy_(alg.log_block(), non_blocking=True)      # opt_state (+ the sums of the options that are on): one copy
        pin["ls"][slot].copy_(env._buf.log_stats, non_blocking=True)
        pin["std"][slot].copy_(self._noise_std(alg.actor_critic).mean().reshape(1), non_blocking=True)
        comm_words = alg.comm_status_snapshot(slot)
        env._buf.clear_log_sums()
        done = torch.cuda.Event()
        done.record()
        return dict(slot=slot, done=done, comm=comm_words)

    @staticmethod
    def _noise_std(ac):
        """The policy's standard deviations: `noise_std` (sigma whichever way it is parametrised), else the reference's `std`."""
        s = getattr(ac, "noise_std", None)
        return (ac.std if s is None else s).detach()

    def _log_flush(self, pending, num_learning_iterations):
        """Print / record the log block of a finished iteration from its host snapshot (no device access: the device is busy with
        the next iteration)."""
        import hgym
        from humanoid.envs.base.legged_robot import KERNEL_REWARD_TERMS
        snap, ev = pending["snap"], pending["ev"]
        snap["done"].synchronize()
        if snap.get("comm") is not None:       # N > 1 with the direct gradient exchange: an expired wait must not go unnoticed
            self.alg.check_comm(snap["comm"].tolist())
        if snap.get("diag") is not None:
            self._diag_publish(pending["it"], snap["diag"])
        pin, slot = self._log_pin, snap["slot"]
        o = self.alg.read_log(pin["opt"][slot])      # (also leaves the options' losses where log() finds them: alg.log_scalars())
        ep, returns, lengths = hgym.log_stats_summary(pin["ls"][slot], self.env.reward_names, KERNEL_REWARD_TERMS)
        collection_time, learn_time = ev[0].elapsed_time(ev[1]) * 1e-3, ev[1].elapsed_time(ev[2]) * 1e-3
        self.last_collection_time, self.last_learn_time = collection_time, learn_time
        self.log(dict(it=pending["it"], num_learning_iterations=num_learning_iterations, collection_time=collection_time,
                      learn_time=learn_time, mean_value_loss=o["mean_value_loss"], mean_surrogate_loss=o["mean_surrogate_loss"], ep_infos=[ep],
                      rewbuffer=deque(returns, maxlen=100), lenbuffer=deque(lengths, maxlen=100),
                      learning_rate=o["learning_rate"], mean_std=float(pin["std"][slot][0])))

    def log(self, locs, width=80, pad=35):
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
        iteration_time = locs["collection_time"] + locs["learn_time"]
        self.tot_time += iteration_time
        scal = (lambda *a: self.writer.add_scalar(*a)) if self.writer is not None else (lambda *a: None)
        ep_string = ""
        if locs["ep_infos"]:
            for key in locs["ep_infos"][0]:
                if all(isinstance(e[key], float) for e in locs["ep_infos"]):        # the device-side log sink hands in host numbers
                    value = sum(e[key] for e in locs["ep_infos"]) / len(locs["ep_infos"])
                else:
                    vals = torch.stack([torch.as_tensor(e[key], device=self.device).float().reshape(()) for e in locs["ep_infos"]])
                    value = float(vals.mean())
                scal("Episode/" + key, value, locs["it"])
                ep_string += f"""{f'Mean episode {key}:':>{pad}} {value:.4f}\n"""
        mean_std = locs["mean_std"] if "mean_std" in locs else float(self._noise_std(self.alg.actor_critic).mean())
        learning_rate = locs["learning_rate"] if "learning_rate" in locs else self.alg.learning_rate
        fps = int(self.num_steps_per_env * self.env.num_envs / iteration_time)
        options = self.alg.log_scalars()      # the losses of the options that are on, in the order they are written
        opt = dict(options)
        behavior = opt.get("Loss/behavior")
        if behavior is not None:      # Distillation.update() hands its loss back in the surrogate's place; a cloning run has no surrogate
            locs = dict(locs, mean_surrogate_loss=0.0)
        scal("Loss/value_function", locs["mean_value_loss"], locs["it"])
        scal("Loss/surrogate", locs["mean_surrogate_loss"], locs["it"])
        scal("Loss/learning_rate", learning_rate, locs["it"])
        for tag, value in options:
            scal(tag, value, locs["it"])
        scal("Policy/mean_noise_std", mean_std, locs["it"])
        scal("Perf/total_fps", fps, locs["it"])
        scal("Perf/collection time", locs["collection_time"], locs["it"])
        scal("Perf/learning_time", locs["learn_time"], locs["it"])
        have_eps = len(locs["rewbuffer"]) > 0
        if have_eps:
            scal("Train/mean_reward", statistics.mean(locs["rewbuffer"]), locs["it"])
            scal("Train/mean_episode_length", statistics.mean(locs["lenbuffer"]), locs["it"])
            scal("Train/mean_reward/time", statistics.mean(locs["rewbuffer"]), self.tot_time)
            scal("Train/mean_episode_length/time", statistics.mean(locs["lenbuffer"]), self.tot_time)
        head = f" \033[1m Learning iteration {locs['it']}/{self.current_learning_iteration + locs['num_learning_iterations']} \033[0m "
        out = (f"""{'#' * width}\n{head.center(width, ' ')}\n\n"""
               f"""{'Computation:':>{pad}} {fps:.0f} steps/s (collection: {locs['collection_time']:.3f}s, learning {locs['learn_time']:.3f}s)\n"""
               f"""{'Value function loss:':>{pad}} {locs['mean_value_loss']:.4f}\n"""
               f"""{'Surrogate loss:':>{pad}} {locs['mean_surrogate_loss']:.4f}\n"""
               f"""{'Mean action noise std:':>{pad}} {mean_std:.2f}\n""")
        if behavior is not None:
            out += f"""{'Behavior loss:':>{pad}} {behavior:.6f}\n"""
        if "Loss/rnd" in opt:
            out += (f"""{'RND predictor loss:':>{pad}} {opt['Loss/rnd']:.6f}\n"""
                    f"""{'Mean intrinsic reward:':>{pad}} {opt['Rnd/intrinsic_reward']:.6f} (weight {opt['Rnd/weight']:.4g})\n""")
        if have_eps:
            out += (f"""{'Mean reward:':>{pad}} {statistics.mean(locs['rewbuffer']):.2f}\n"""
                    f"""{'Mean episode length:':>{pad}} {statistics.mean(locs['lenbuffer']):.2f}\n""")
        out += ep_string
        done = locs["it"] + 1 - self.current_learning_iteration
        eta = self.tot_time / max(done, 1) * (locs["num_learning_iterations"] - done)
        out += (f"""{'-' * width}\n{'Total timesteps:':>{pad}} {self.tot_timesteps}\n"""
                f"""{'Iteration time:':>{pad}} {iteration_time:.2f}s\n{'Total time:':>{pad}} {self.tot_time:.2f}s\n"""
                f"""{'ETA:':>{pad}} {eta:.1f}s\n""")
        print(out)

    def invalidate_graph(self):
        """Drop the captured rollout; the next learn() iteration runs eagerly and the one after re-captures."""
        self._rollout_capture, self._update_capture = _CapturedGraph(), _CapturedGraph()

    env_state_path = staticmethod(ckpt.env_state_path)

    def save(self, path, infos=None, wait=True, env_state=False, iterations_done=None):
        """on_policy_runner.py:274-281 (same dict, same keys).

        env_state=True (learn() passes it when cfg["exact_resume"] is set; `python scripts/train.py` sets that from HGYM_EXACT_RESUME=1)
        also writes the sidecar env_state_path(path), envstate_<it>.pt: {"env": env.state_dict(), "iterations_done", "num_steps_per_env",
        "world_size", "rank"} -- with model_<it>.pt everything load() needs to CONTINUE the run bit for bit (see load()).
        iterations_done: the true number of finished iterations (default current_learning_iteration; learn() passes it + 1 for an
        in-loop checkpoint, whose "iter" is the stale value the reference writes).  model_<it>.pt itself is unchanged: same four keys,
        same bytes.  The sidecar is renamed into place BEFORE the model file, so a visible model_<it>.pt of such a run has its sidecar.
        On the background path the env snapshot follows the parameters': stream-ordered copies into two alternating pinned host sets,
        the file written by the same writer job.

        wait=True (the reference's semantics, and what a direct caller gets): the file is on disk when the call returns.  learn() passes
        wait=False for ALL its checkpoints, the final one included: on the background path (humanoid/algo/ppo/checkpoint.py, which also
        holds the measurements) the file of the last iteration is complete a few milliseconds AFTER learn() returns -- `wait_for_saves()`
        (called by load(), by the next save(wait=True), and at interpreter exit, which is when scripts/train.py ends) waits for it.  A
        caller that reads model_<it>.pt from the same process right after learn() calls runner.wait_for_saves() first."""
        t0 = time.time()
        alg, it = self.alg, self.current_learning_iteration
        extra = dict(iterations_done=int(it if iterations_done is None else iterations_done), num_steps_per_env=int(self.num_steps_per_env),
                     world_size=int(getattr(alg, "_world", 1)), rank=int(getattr(alg, "_rank", 0))) if env_state else None
        if not ckpt.background_eligible(alg, self.device):
            side = dict(env={k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.env.state_dict().items()}, **extra,
                        **ckpt.sidecar_entries(alg)) if env_state else None
            ckpt.write_checkpoint({"model_state_dict": alg.actor_critic.state_dict(), "optimizer_state_dict": alg.optimizer.state_dict(),
                                   "iter": it, "infos": infos, **ckpt.extra_entries(alg)}, path, side)
        else:
            if getattr(self, "_snapshot", None) is None:
                self._snapshot = ckpt.Snapshot(alg.net)
            # PPO.exploration_noise: the AR(1) state rides in the sidecar; its copy is enqueued ahead of the snapshot's event
            side_extra = ckpt.sidecar_entries(alg, buf=self._snapshot.next_set()) if env_state else {}
            vn = getattr(alg, "value_normalizer", None)      # PPO.value_normalization: its three doubles ride in the snapshot
            shot = self._snapshot.take(alg.net, alg.actor_critic, self.env if env_state else None,
                                       value_norm=None if vn is None else (vn.block, vn.eps))
            if getattr(alg, "_guide", None) is not None:      # PPO.guidance: host data, formed here where the count is this checkpoint's
                shot["guidance"] = alg._guide.state_dict()
            if getattr(alg, "_warmup", None) is not None:      # PPO.critic_warmup_updates: host data, likewise
                shot["critic_warmup"] = alg._warmup.state_dict()
            side = dict(env=shot["env"], **extra, **side_extra) if env_state else None
            ckpt.WRITER.submit(lambda: ckpt.write_snapshot(shot, type(alg.optimizer).HYPER, it, infos, path, side))
            if wait:
                ckpt.WRITER.wait()
        self.save_time_s = getattr(self, "save_time_s", 0.0) + (time.time() - t0)     # host time the TRAINING thread spent in checkpoints (bench.py reports it)

    def wait_for_saves(self):
        """Block until every checkpoint handed to the background writer is on disk (re-raises a writer error)."""
        t0 = time.time()
        ckpt.WRITER.wait()
        self.save_time_s = getattr(self, "save_time_s", 0.0) + (time.time() - t0)

    def load(self, path, load_optimizer=True, env_state=None):
        """on_policy_runner.py:283-290, plus the generators' counters (PPO.seek, LeggedRobot.seek).

        With a sidecar -- envstate_<it>.pt beside `path` (env_state_path), or env_state=<its path>; env_state=False ignores one -- the
        run CONTINUES: the iteration count becomes the sidecar's iterations_done (the true one, not the model file's "iter"),
        PPO.seek() gets that count, the env is restored with env.load_state_dict() (its own counters included, so LeggedRobot.seek is
        not called), and the next learn(..., init_at_random_ep_len=True) keeps the restored episode lengths, once.  With parameters and
        Adam's state loaded as well, the iterations that follow compute bit for bit what the saved run computed after that checkpoint
        (tests/test_exact_resume_gpu.py).  The optimiser: loaded when load_optimizer is true, and regardless of it when the run asked for
        cfg["exact_resume"]; a plain load(path, load_optimizer=False) keeps its meaning.

        Scope.  Exact for PPO.permutation = "device" (the default) on one rank: with "torch" the minibatch permutation comes from
        torch's global generator, which the sidecar does not carry; a data-parallel run says once that it ignores the sidecar and resumes as without it.
        The log sink's rings and the host's rewbuffer / lenbuffer are logging state, zeroed at every learn(): the first log blocks
        after a resume average over fewer episodes.  An evaluation env (set_eval_env) is not touched.  Without a sidecar: as ever."""
        ckpt.WRITER.wait()                      # a checkpoint this process is still writing
        alg, ac, loaded = self.alg, self.alg.actor_critic, None
        if isinstance(ac, StudentTeacher):
            # a distillation run: a checkpoint without `teacher.*` entries is the TEACHER's PPO checkpoint (StudentTeacher.load_state_dict):
            # its weights become the teacher, and nothing else of it -- no optimiser state, no env sidecar, iteration 0
            loaded = torch.load(path, map_location=self.device)
            if not any(k.startswith("teacher.") for k in loaded["model_state_dict"]):
                ac.load_state_dict(loaded["model_state_dict"])
                self.current_learning_iteration = 0
                return loaded.get("infos")
        side, side_path = None, ckpt.resolve_sidecar(path, env_state, getattr(alg, "_world", 1), self)
        if side_path is not None:
            side = torch.load(side_path, map_location="cpu")
            ckpt.check_sidecar(side, self.num_steps_per_env, self.env, alg)      # (refused before anything is changed)
        if loaded is None:
            loaded = torch.load(path, map_location=self.device)
        ckpt.check_compatible(loaded, ac, alg._rnd, os.path.basename(str(path)), value_norm=ckpt.value_norm_spec(alg),
                              guidance=getattr(alg, "_guide", None), critic_warmup=getattr(alg, "_warmup", None) is not None)
        if getattr(alg, "_warmup", None) is not None:
            alg._warmup.load_state_dict(loaded[ckpt.WARMUP_KEY])
        if getattr(alg, "_guide", None) is not None:
            alg._guide.load_state_dict(loaded[ckpt.GUIDE_KEY])
        if getattr(alg, "value_normalizer", None) is not None:
            alg.value_normalizer.load_state_dict(loaded[ckpt.VALUE_NORM_KEY])
        if alg._rnd is not None:
            alg._rnd.load_rnd_state_dict(loaded[RND_STATE_KEY])
        if getattr(ac, "empirical_normalization", False):        # the statistics first, then the parameters (whose load refolds the first layers with them)
            alg.net.load_norm_state(dict(obs=loaded[NORM_KEYS[0]], critic_obs=loaded[NORM_KEYS[1]]))
        ac.load_state_dict(loaded["model_state_dict"])
        if load_optimizer or (side is not None and self.cfg.get("exact_resume", False)):
            alg.optimizer.load_state_dict(loaded["optimizer_state_dict"])
        self.current_learning_iteration = loaded["iter"] if side is None else int(side["iterations_done"])
        if hasattr(alg, "seek"):
            alg.seek(self.current_learning_iteration, self.num_steps_per_env)
        if side is not None:
            self.env.load_state_dict(side["env"])
            ckpt.load_sidecar_entries(side, alg)      # PPO.exploration_noise: the AR(1) state the next rollout's table starts from
            self._keep_episode_lengths = True
        elif hasattr(self.env, "seek"):       # the env's draw streams (commands, pushes, noise, resets) continue as well
            self.env.seek(self.current_learning_iteration, self.num_steps_per_env)
        return loaded["infos"]

    def get_inference_policy(self, device=None):
        self.alg.actor_critic.eval()
        if device is not None and str(device) != str(self.device):
            import copy
            if not getattr(self.alg.actor_critic, "empirical_normalization", False):
                return copy.deepcopy(self.alg.actor_critic.actor).to(device)
            actor = copy.deepcopy(self.alg.actor_critic.actor).to("cpu")      # raw observations in: the folded first layer
            W, b = self.alg.actor_critic.folded_first_layer(0)
            with torch.no_grad():
                actor[0].weight.copy_(W)
                actor[0].bias.copy_(b)
            return actor.to(device)
        return self.alg.actor_critic.act_inference

    def get_inference_critic(self, device=None):
        self.alg.actor_critic.eval()
        return self.alg.actor_critic.evaluate
