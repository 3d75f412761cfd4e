"""Random Network Distillation (rsl_rl's rnd_cfg): an intrinsic exploration reward for PPO on the MI355X hot path.

A frozen, randomly initialised `target` MLP embeds a slice of the observations; a `predictor` MLP is trained to reproduce the embedding on
the states the policy visits.  Where the predictor is still wrong the state is new, and the error -- normalised by a running deviation
and weighted by a schedule -- is added to the stored rewards ahead of GAE (hgym_rnd_rewards).  Nothing inside a rollout consumes the
intrinsic reward, so the whole pass runs once behind the rollout, over the stored rows, as the deferred critic and a teacher's pass do.

On the device both nets live in a hgym.NetBuffers of their own, in the actor slot beside a placeholder critic (StudentTeacher's scheme):
the target only ever runs hgym_mlp_forward; the predictor is trained by hgym_bc_grad (MSE) + hgym_ppo_apply, Distillation's step.

Set `PPO.rnd = RandomNetworkDistillation(...)` before init_storage (OnPolicyRunner does it from train_cfg["algorithm"]["rnd_cfg"]).
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .actor_critic import _mlp
from .student_teacher import PLACEHOLDER_CRITIC_DIMS, TEACHER_MAX_BATCH, forward_in_pieces

NO_CLIP = 3.0e38      # a clip that never binds (Distillation's)
MAX_OUTPUTS = 12      # the embedding is the `actor` head of a NetBuffers, which carries at most 12 outputs (the reward kernel takes 64)
SCHEDULES = ("constant", "step", "linear")
STATE_SOURCES = ("critic_obs", "obs")
STATE_NORM_EPS = 1e-2      # as for empirical_normalization

DEFAULTS = dict(weight=0.0, weight_schedule=None, reward_normalization=True, state_normalization=False, num_outputs=12,
                predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128], learning_rate=1e-3, gamma=0.99, state=None)
STATE_DICT_KEYS = ("predictor", "target", "predictor_adam_m", "predictor_adam_v", "predictor_opt_state", "block", "num_envs", "state_norm")


def _weight(name, v):
    w = _number(name, v)
    if not (w >= 0.0 and math.isfinite(w)):
        raise ValueError("rnd_cfg.%s=%r: must be finite and >= 0" % (name, v))
    return w


def _number(name, v):
    """v as a float, or ValueError naming the key: a bool, a string, None or anything float() refuses is not a number here."""
    if not (isinstance(v, (bool, str, bytes)) or v is None):
        try:
            return float(v)
        except (TypeError, ValueError):
            pass
    raise ValueError("rnd_cfg.%s=%r: a number is needed" % (name, v))


def _step(name, v):
    x = _number("weight_schedule." + name, v)
    if not (math.isfinite(x) and x == int(x) and x >= 0):
        raise ValueError("rnd_cfg.weight_schedule.%s=%r: must be an integer >= 0" % (name, v))
    return int(x)


def parse_schedule(weight, sched):
    """(weight, weight_schedule) of an rnd_cfg -> dict(mode, weight, final_value, initial_step, final_step), checked.
    weight_schedule: None or {"mode": "constant"}; {"mode": "step", "final_step", "final_value"}; {"mode": "linear", "initial_step",
    "final_step", "final_value"} with final_step > initial_step.  ValueError naming the key for anything else."""
    w0 = _weight("weight", weight)
    out = dict(mode="constant", weight=w0, final_value=w0, initial_step=0, final_step=0)
    if sched is None:
        return out
    if not isinstance(sched, dict) or "mode" not in sched:
        raise ValueError("rnd_cfg.weight_schedule=%r: a dict with a \"mode\" (%s) is needed" % (sched, ", ".join(SCHEDULES)))
    mode = sched["mode"]
    if mode not in SCHEDULES:
        raise ValueError("rnd_cfg.weight_schedule.mode=%r: one of %s" % (mode, ", ".join(SCHEDULES)))
    allowed = dict(constant=(), step=("final_step", "final_value"), linear=("initial_step", "final_step", "final_value"))[mode]
    unknown = sorted(set(sched) - {"mode"} - set(allowed))
    if unknown:
        raise ValueError("rnd_cfg.weight_schedule: unknown key %s for mode %r (%s)" % (", ".join(unknown), mode, ", ".join(allowed) or "none"))
    missing = [k for k in allowed if k not in sched]
    if missing:
        raise ValueError("rnd_cfg.weight_schedule: mode %r needs %s" % (mode, ", ".join(missing)))
    out["mode"] = mode
    if mode != "constant":
        out["final_value"] = _weight("weight_schedule.final_value", sched["final_value"])
        out["final_step"] = _step("final_step", sched["final_step"])
    if mode == "linear":
        out["initial_step"] = _step("initial_step", sched["initial_step"])
        if out["final_step"] <= out["initial_step"]:
            raise ValueError("rnd_cfg.weight_schedule: final_step=%d must be greater than initial_step=%d" % (out["final_step"], out["initial_step"]))
    return out


def schedule_weight(s, c):
    """The weight of step count c under a parse_schedule() dict, as hgym_rnd_rewards evaluates it (python doubles, left to right)."""
    c = int(c)
    if s["mode"] == "step":
        return s["weight"] if c < s["final_step"] else s["final_value"]
    if s["mode"] == "linear":
        if c <= s["initial_step"]:
            return s["weight"]
        if c >= s["final_step"]:
            return s["final_value"]
        return s["weight"] + (s["final_value"] - s["weight"]) * float(c - s["initial_step"]) / float(s["final_step"] - s["initial_step"])
    return s["weight"]


def _hidden(name, v):
    if not isinstance(v, (list, tuple)) or not v or any(isinstance(d, bool) or not isinstance(d, int) or d < 1 for d in v):
        raise ValueError("rnd_cfg.%s=%r: a non-empty list of positive widths" % (name, v))
    return [int(d) for d in v]


def parse_config(cfg, num_obs, num_critic_obs, critic_frame=None):
    """An rnd_cfg dict -> the complete, checked configuration (a new dict with every key of DEFAULTS; `schedule` = parse_schedule();
    `state` resolved to (source, start, stop)).  Keys: rsl_rl's weight, weight_schedule, reward_normalization (default True),
    state_normalization (default False), num_outputs, predictor_hidden_dims, target_hidden_dims, learning_rate; this repository's gamma
    (0.99, the discount of the per-env average the reward is normalised by) and state.  Any other key: ValueError naming it.

    state = (source, start, stop): the contiguous column range [start, stop) of "critic_obs" or "obs" that both nets embed.  Default: the
    NEWEST privileged frame of critic_obs.  The env stacks frames oldest -> newest, so with c_frame_stack = 3 frames of 73 columns that
    is critic_obs[:, 146:219] -- ("critic_obs", num_critic_obs - critic_frame, num_critic_obs); without a frame width the whole row."""
    if not isinstance(cfg, dict):
        raise ValueError("rnd_cfg=%r: a dict is needed" % (cfg,))
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise ValueError("rnd_cfg: unknown key %s (known: %s)" % (", ".join(map(str, unknown)), ", ".join(DEFAULTS)))
    c = dict(DEFAULTS, **cfg)
    c["schedule"] = parse_schedule(c["weight"], c["weight_schedule"])
    c["weight"] = c["schedule"]["weight"]
    for k in ("reward_normalization", "state_normalization"):
        if not isinstance(c[k], bool):
            raise ValueError("rnd_cfg.%s=%r: True or False" % (k, c[k]))
    K = _number("num_outputs", c["num_outputs"])
    if not (math.isfinite(K) and K == int(K) and 1 <= K <= MAX_OUTPUTS):
        raise ValueError("rnd_cfg.num_outputs=%r: an integer in [1, %d] (the embedding is a NetBuffers head)" % (c["num_outputs"], MAX_OUTPUTS))
    c["num_outputs"] = int(K)
    c["predictor_hidden_dims"] = _hidden("predictor_hidden_dims", c["predictor_hidden_dims"])
    c["target_hidden_dims"] = _hidden("target_hidden_dims", c["target_hidden_dims"])
    lr = _number("learning_rate", c["learning_rate"])
    if not (lr > 0.0 and math.isfinite(lr)):
        raise ValueError("rnd_cfg.learning_rate=%r: must be finite and > 0" % (c["learning_rate"],))
    c["learning_rate"] = lr
    g = _number("gamma", c["gamma"])
    if not (0.0 <= g < 1.0):
        raise ValueError("rnd_cfg.gamma=%r: must lie in [0, 1)" % (c["gamma"],))
    c["gamma"] = g
    widths = dict(obs=int(num_obs), critic_obs=int(num_critic_obs))
    st = c["state"]
    if st is None:
        f = int(critic_frame) if critic_frame else widths["critic_obs"]
        st = ("critic_obs", widths["critic_obs"] - f, widths["critic_obs"])
    if not isinstance(st, (list, tuple)) or len(st) != 3 or st[0] not in STATE_SOURCES:
        raise ValueError("rnd_cfg.state=%r: (source, start, stop) with source one of %s (a list of scattered columns is not supported)"
                         % (st, ", ".join(STATE_SOURCES)))
    src, a, b = st
    if any(isinstance(x, bool) or not isinstance(x, int) for x in (a, b)) or not (0 <= a < b <= widths[src]):
        raise ValueError("rnd_cfg.state=%r: columns [start, stop) must lie inside the %d columns of %s" % (st, widths[src], src))
    c["state"] = (src, int(a), int(b))
    return c


def check_setup(world=1, symmetry=None, symmetry_augmentation=True, distillation=False):
    """What PPO.init_storage refuses with RND on, as a function that needs no device (ValueError each; DESIGN.md section 27 names each as a
    follow-up): more than one rank (the predictor's gradient would need its own exchange); symmetry augmentation (the drawn rows include
    mirrored ones, which have no RND state -- the mirror loss without augmentation is fine); Distillation."""
    if int(world) > 1:
        raise ValueError("PPO.rnd runs on one rank (world size %d): the predictor's gradient has no exchange" % int(world))
    if symmetry is not None and bool(symmetry_augmentation):
        raise ValueError("PPO.rnd does not support PPO.symmetry_augmentation: mirrored rows have no RND state (the mirror loss without augmentation is fine)")
    if distillation:
        raise ValueError("PPO.rnd does not support Distillation: a cloning run has no rewards to add to")


def check_state_dict(sd, name, has_rnd, num_envs=None):
    """OnPolicyRunner.load's refusals, by name: a checkpoint with rnd_state_dict for a run without RND, the reverse, and another num_envs
    (the per-env average G is part of the state).  sd: the checkpoint's rnd_state_dict or None."""
    if sd is not None and not has_rnd:
        raise RuntimeError("%s carries rnd_state_dict (it was trained with RND); this run has no rnd_cfg" % name)
    if sd is None and has_rnd:
        raise RuntimeError("%s has no rnd_state_dict; this run was configured with rnd_cfg" % name)
    if sd is not None:
        missing = [k for k in STATE_DICT_KEYS if k not in sd]
        if missing:
            raise RuntimeError("%s: rnd_state_dict lacks %s" % (name, ", ".join(missing)))
        if num_envs is not None and int(sd["num_envs"]) != int(num_envs):
            raise RuntimeError("%s: rnd_state_dict holds the per-env average of %d envs, this run has %d" % (name, int(sd["num_envs"]), int(num_envs)))


class RandomNetworkDistillation(nn.Module):
    def __init__(self, num_obs, num_critic_obs, cfg=None, critic_frame=None, activation=None, seed=None):
        """cfg: an rnd_cfg dict (parse_config).  seed: both nets are initialised from a generator of their own seeded with it (default:
        torch.initial_seed(), the run's seed), so a run is reproducible whatever was drawn before."""
        super().__init__()
        self.cfg = parse_config(dict(cfg or {}), num_obs, num_critic_obs, critic_frame)
        self.activation = activation if activation is not None else nn.ELU()
        self.source, self.start, self.stop = self.cfg["state"]
        self.num_states, self.num_outputs = self.stop - self.start, self.cfg["num_outputs"]
        self.predictor = _mlp([self.num_states] + self.cfg["predictor_hidden_dims"] + [self.num_outputs], self.activation)
        self.target = _mlp([self.num_states] + self.cfg["target_hidden_dims"] + [self.num_outputs], self.activation)
        g = torch.Generator().manual_seed(int(torch.initial_seed() if seed is None else seed) & 0x7FFFFFFFFFFFFFFF)
        with torch.no_grad():
            for seq in (self.predictor, self.target):      # nn.Linear's own ranges, drawn from `g`
                for m in seq:
                    if isinstance(m, nn.Linear):
                        bound = 1.0 / math.sqrt(m.in_features)
                        m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2.0 - 1.0) * bound)
                        m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2.0 - 1.0) * bound)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.nets = None      # bind(): (predictor NetBuffers, target NetBuffers)
        self.block = self.sums = None
        self.last_loss = None
        self.last_log = None

    bound = property(lambda self: self.nets is not None)

    # ------------------------------------------------------------------ binding to the HIP path
    def bind(self, precision, max_batch, device, num_envs):
        """Two NetBuffers -- the MLP in the actor slot, PLACEHOLDER_CRITIC_DIMS beside it, a valid sigma, sync_shadow() -- the way
        StudentTeacher.bind builds the teacher's.  The predictor's takes minibatches of max_batch rows and has its own learning rate;
        the target only runs forwards, in pieces.  Also the reward pass's state block (num_envs) and the loss's two sums."""
        import hgym
        from hgym import _lib as L
        S, K = self.num_states, self.num_outputs
        nets = []
        for seq, hidden, mb, lr in ((self.predictor, self.cfg["predictor_hidden_dims"], int(max_batch), self.cfg["learning_rate"]),
                                    (self.target, self.cfg["target_hidden_dims"], min(int(max_batch), TEACHER_MAX_BATCH), 0.0)):
            ncfg = hgym.make_net_config(S, S, K, hidden, PLACEHOLDER_CRITIC_DIMS, precision, mb, activation=self.activation)
            nb = hgym.NetBuffers(ncfg, device, learning_rate=lr)
            nb.params[:K] = 1.0      # a valid sigma; nothing reads it
            with torch.no_grad():
                for name, p in seq.named_parameters():
                    view = nb.views["actor." + name]
                    view.copy_(p.detach().to(view.device))
                    p.data = view
            nb.sync_shadow()
            nets.append(nb)
        self.nets = tuple(nets)
        self.num_envs = int(num_envs)
        self.block = L.rnd_block(num_envs, device)
        self.sums = torch.zeros(2, dtype=torch.float64, device=device)
        s = self.cfg["schedule"]
        self.rnd_cfg = L.RndConfig(self.cfg["gamma"], s["weight"], s["final_value"], s["initial_step"], s["final_step"],
                                   SCHEDULES.index(s["mode"]), 1 if self.cfg["reward_normalization"] else 0)
        self._bc_cfg = hgym.make_bc_config("mse")
        self._apply_cfg = hgym.make_ppo_config(max_grad_norm=NO_CLIP, desired_kl=0.0, adaptive=False, world_size=1, grad_norm_ready=False)
        # state normalisation: running fp64 statistics in torch on the device, and the fp32 pair the copy applies
        self.norm = None
        if self.cfg["state_normalization"]:
            z = lambda v, dt: torch.full((S,), v, dtype=dt, device=device)
            self.norm = dict(mean=z(0.0, torch.float64), var=z(1.0, torch.float64), count=torch.zeros(1, dtype=torch.float64, device=device),
                             m=z(0.0, torch.float32), s=z(1.0 / (1.0 + STATE_NORM_EPS), torch.float32))
        return self

    def _source(self, storage):
        src = storage._priv_all if self.source == "critic_obs" else storage._obs_all
        if src is None:
            raise ValueError("rnd_cfg.state names critic_obs, but the env has no privileged observations")
        return src[:, :, self.start:self.stop]

    # ------------------------------------------------------------------ the pass behind a rollout
    def reward_pass(self, storage, last_critic_obs=None, last_obs=None, slot_T_written=True):
        """Ahead of GAE: the contiguous (normalised) copy of the chosen columns of slots 0 .. T, the target over rows 0 .. T, the predictor
        over rows 1 .. T (the NEXT state of every transition), hgym_rnd_rewards into storage.rewards.  Fixed launches and arguments.

        Slot T is the state behind the last transition.  The zero-copy and fused rollouts have the env write it into the storage; on the
        plain path (act / process_env_step with the env's own tensors) add_transitions fills slots 0 .. T - 1 only, and the caller's
        bootstrap observation -- compute_returns' last_critic_obs, or last_obs for a state taken from "obs" -- is copied into row T of
        rnd_states here.  slot_T_written False and no such observation: RuntimeError, because the storage's slot T is then stale."""
        from hgym import _lib as L
        st = storage
        T, N = st.num_transitions_per_env, st.num_envs
        from_priv = self.source == "critic_obs" and st._priv_all is not None
        last = last_critic_obs if (from_priv or st._priv_all is None) else last_obs
        slot = (st._priv_all if from_priv else st._obs_all)[T]
        external = last is not None and last.data_ptr() != slot.data_ptr()
        if last is None and not slot_T_written:
            raise RuntimeError("PPO.rnd: the state behind the last transition is not in the storage (the rollout wrote slots 0 .. T - 1 only) and "
                               "rnd_cfg.state reads %r: call compute_returns(last_critic_obs, last_obs=<the env's last observations>)" % self.source)
        with torch.inference_mode():
            st.rnd_states.copy_(self._source(st))
            if external:
                st.rnd_states[T].copy_(last[:, self.start:self.stop])
            if self.norm is not None:
                st.rnd_states.sub_(self.norm["m"]).mul_(self.norm["s"])
        pred_net, target_net = self.nets
        forward_in_pieces(target_net, st.rnd_states.flatten(0, 1), st.rnd_target.flatten(0, 1))
        forward_in_pieces(pred_net, st.rnd_states[1:].flatten(0, 1), st.rnd_pred.flatten(0, 1))
        L.check(L.lib.hgym_rnd_rewards(T, N, self.num_outputs, L.fptr(st.rnd_pred), L.fptr(st.rnd_target[1:]), L.fptr(st.rewards),
                                       L.fptr(st.rnd_error), L.fptr(st.rnd_intrinsic), C.byref(self.rnd_cfg), L.f64ptr(self.block),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_rnd_rewards")

    # ------------------------------------------------------------------ the predictor's training
    def begin_update(self):
        self.sums[0:2] = 0.0      # (a slice: a fill kernel)

    def train_step(self, storage, idx):
        """One predictor step on the rows `idx` of slots 0 .. T - 1 against rnd_target[:T]: hgym_bc_grad (MSE) + hgym_ppo_apply."""
        import hgym
        T = storage.num_transitions_per_env
        net = self.nets[0]
        batch = hgym.make_bc_batch(storage.rnd_states[:T].flatten(0, 1), idx)
        net.bc_grad(self._bc_cfg, batch, storage.rnd_target[:T].flatten(0, 1), self.sums)
        net.ppo_apply(self._apply_cfg)

    def end_update(self, storage):
        """With state_normalization: merge the RAW states of slots 0 .. T - 1 into the running statistics (one batch, the merge formula of
        include/hgym.h), once per update and at its end -- the embeddings the rewards used and the ones the predictor trained on saw the
        same statistics."""
        if self.norm is None:
            return
        nz, T = self.norm, storage.num_transitions_per_env
        with torch.inference_mode():
            x = self._source(storage)[:T].flatten(0, 1).double()
            nb = float(x.shape[0])
            mu_b = x.mean(0)
            var_b = ((x * x).mean(0) - mu_b * mu_b).clamp_(min=0.0)
            nz["count"].add_(nb)
            rate = nb / nz["count"]
            d = mu_b - nz["mean"]
            nz["mean"].add_(rate * d)
            nz["var"].add_(rate * (var_b - nz["var"] + d * (mu_b - nz["mean"])))
            nz["m"].copy_(nz["mean"])
            nz["s"].copy_(1.0 / (nz["var"].sqrt() + STATE_NORM_EPS))

    def graph_key(self):
        """PPO.update_graph_key's entry: the nets, the block and the configuration bytes the captured launches name."""
        return dict(rnd=(id(self), id(self.nets[0]), id(self.nets[1]), self.block.data_ptr(),
                         bytes(C.string_at(C.addressof(self.rnd_cfg), C.sizeof(self.rnd_cfg)))))

    # ------------------------------------------------------------------ logging
    LOG_DOUBLES = 2 + 16      # the loss's two sums, then the head of the block

    def log_parts(self):
        """The two adjacent parts of PPO's log block (LogBlock.add), together log_tail()'s layout."""
        from hgym import _lib as L
        return ("rnd_sums", self.sums), ("rnd_block", self.block[:L.RND_HEADER])

    def log_tail(self):
        return torch.cat([t for _, t in self.log_parts()])

    def log_from(self, tail):
        """The log numbers from a host copy of log_tail(): Loss/rnd (mean MSE per predictor step) and the block's sums as per-row means."""
        from hgym import _lib as L
        t = [float(v) for v in tail]
        rows = max(t[2 + L.RND_ROWS], 1.0)
        self.last_loss = t[0] / max(t[1], 1.0)
        self.last_log = {"Loss/rnd": self.last_loss, "Rnd/intrinsic_reward": t[2 + L.RND_SUM_INTRINSIC] / rows,
                         "Rnd/extrinsic_reward": t[2 + L.RND_SUM_REWARDS] / rows, "Rnd/weight": t[2 + L.RND_WEIGHT_LAST], "Rnd/std": t[2 + L.RND_STD]}
        return self.last_log

    def read_log(self, parts):
        """log_from() on the two parts of a host copy of PPO.log_block()."""
        return self.log_from(torch.cat((parts["rnd_sums"], parts["rnd_block"])))

    def log_scalars(self):      # Loss/rnd, Rnd/intrinsic_reward, Rnd/extrinsic_reward, Rnd/weight, Rnd/std
        return [] if self.last_log is None else list(self.last_log.items())

    # ------------------------------------------------------------------ checkpoints
    def rnd_state_dict(self):
        """Everything the feature adds to a run: both nets, the predictor's Adam moments and opt_state, the reward pass's block (running
        statistics, step counter, per-env G) and the state normaliser (None when off).  Host tensors."""
        cpu = lambda t: t.detach().cpu().clone()
        sd = dict(predictor={k: cpu(v) for k, v in self.predictor.state_dict().items()},
                  target={k: cpu(v) for k, v in self.target.state_dict().items()}, num_envs=int(getattr(self, "num_envs", 0)),
                  predictor_adam_m=None, predictor_adam_v=None, predictor_opt_state=None, block=None, state_norm=None)
        if self.bound:
            p = self.nets[0]
            sd.update(predictor_adam_m=cpu(p.adam_m), predictor_adam_v=cpu(p.adam_v), predictor_opt_state=cpu(p.opt_state), block=cpu(self.block))
            if self.norm is not None:
                sd["state_norm"] = {k: cpu(self.norm[k]) for k in ("mean", "var", "count")}
        return sd

    def load_rnd_state_dict(self, sd):
        check_state_dict(sd, "rnd_state_dict", True, getattr(self, "num_envs", None) if self.bound else None)
        if (sd["state_norm"] is not None) != (self.bound and self.norm is not None) and self.bound:
            raise RuntimeError("rnd_state_dict: state_normalization is %s in the checkpoint and %s here"
                               % ("on" if sd["state_norm"] is not None else "off", "on" if self.norm is not None else "off"))
        self.predictor.load_state_dict(sd["predictor"])
        self.target.load_state_dict(sd["target"])
        if not self.bound:
            return
        p = self.nets[0]
        with torch.inference_mode():
            for dst, key in ((p.adam_m, "predictor_adam_m"), (p.adam_v, "predictor_adam_v"), (p.opt_state, "predictor_opt_state"), (self.block, "block")):
                dst.copy_(sd[key].to(dst.device))
            if self.norm is not None:
                nz = self.norm
                for k in ("mean", "var", "count"):
                    nz[k].copy_(sd["state_norm"][k].to(nz[k].device))
                nz["m"].copy_(nz["mean"])
                nz["s"].copy_(1.0 / (nz["var"].sqrt() + STATE_NORM_EPS))
        for nb in self.nets:
            nb.sync_shadow()
