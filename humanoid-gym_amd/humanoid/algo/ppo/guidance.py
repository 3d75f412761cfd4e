"""Guidance by a frozen teacher (PPO.guidance): a cloning term inside the PPO loss whose coefficient decays
(kickstarting, Schmitt et al. 2018, with the squared error of the means in place of a KL).  The configuration, the schedule's Python twin
and what init_storage refuses are functions that need no device; Guidance is the option's device side.

PPO.guidance = None | dict with the keys of DEFAULTS:
  teacher              a checkpoint path (model_*.pt), a checkpoint dict, a state dict with `actor.*` entries, or a module (an ActorCritic or
                       its `actor`); None only for a run that load()s a checkpoint carrying the teacher (guidance_state_dict)
  coef                 c >= 0: L += c / (B A) sum (mu - t)^2, t the teacher's mean on the same stored row, detached
  coef_schedule        None or {"mode": "constant"}; {"mode": "step", "final_step", "final_value"}; {"mode": "linear", "initial_step",
                       "final_step", "final_value"} -- rnd.parse_schedule's keys and checks; steps are learning iterations
  teacher_hidden_dims  default: the shapes of the checkpoint's actor.* weights
  teacher_activation   a torch.nn module, or the name of one ("ELU", "Tanh", ..); default: the student's
  teacher_max_batch    rows per launch of the teacher's pass; default: the student's max_batch capped at TEACHER_MAX_BATCH
None, or a schedule that is 0 everywhere: off."""
import math
import os
import struct

import torch

from .student_teacher import PLACEHOLDER_CRITIC_DIMS, TEACHER_MAX_BATCH, forward_in_pieces

DEFAULTS = dict(teacher=None, coef=0.0, coef_schedule=None, teacher_hidden_dims=None, teacher_activation=None, teacher_max_batch=None)
SCHEDULES = ("constant", "step", "linear")
STATE_KEY = "guidance_state_dict"      # what a checkpoint of a run with PPO.guidance carries: count, schedule, teacher (its actor.* tensors)
OBS_NORM_KEY = "obs_norm_state_dict"   # a teacher trained with empirical_normalization carries its statistics under this key


# ------------------------------------------------------------------------------------------------ the schedule
def _number(name, v):
    if not (isinstance(v, (bool, str, bytes)) or v is None):
        try:
            return float(v)
        except (TypeError, ValueError):
            pass
    raise ValueError("PPO.guidance.%s=%r: a number is needed" % (name, v))


def _coef(name, v):
    c = _number(name, v)
    if not (c >= 0.0 and math.isfinite(c)):
        raise ValueError("PPO.guidance.%s=%r: must be finite and >= 0" % (name, v))
    return c


def _step(name, v):
    x = _number("coef_schedule." + name, v)
    if not (math.isfinite(x) and x == int(x) and x >= 0):
        raise ValueError("PPO.guidance.coef_schedule.%s=%r: must be an integer >= 0" % (name, v))
    return int(x)


def parse_schedule(coef, sched):
    """(coef, coef_schedule) -> dict(mode, coef, final_value, initial_step, final_step), checked as rnd.parse_schedule checks its own.
    ValueError naming the key for anything else."""
    c0 = _coef("coef", coef)
    out = dict(mode="constant", coef=c0, final_value=c0, initial_step=0, final_step=0)
    if sched is None:
        return out
    if not isinstance(sched, dict) or "mode" not in sched:
        raise ValueError("PPO.guidance.coef_schedule=%r: a dict with a \"mode\" (%s) is needed" % (sched, ", ".join(SCHEDULES)))
    mode = sched["mode"]
    if mode not in SCHEDULES:
        raise ValueError("PPO.guidance.coef_schedule.mode=%r: one of %s" % (mode, ", ".join(SCHEDULES)))
    allowed = dict(constant=(), step=("final_step", "final_value"), linear=("initial_step", "final_step", "final_value"))[mode]
    unknown = sorted(set(sched) - {"mode"} - set(allowed))
    if unknown:
        raise ValueError("PPO.guidance.coef_schedule: unknown key %s for mode %r (%s)" % (", ".join(unknown), mode, ", ".join(allowed) or "none"))
    missing = [k for k in allowed if k not in sched]
    if missing:
        raise ValueError("PPO.guidance.coef_schedule: mode %r needs %s" % (mode, ", ".join(missing)))
    out["mode"] = mode
    if mode != "constant":
        out["final_value"] = _coef("coef_schedule.final_value", sched["final_value"])
        out["final_step"] = _step("final_step", sched["final_step"])
    if mode == "linear":
        out["initial_step"] = _step("initial_step", sched["initial_step"])
        if out["final_step"] <= out["initial_step"]:
            raise ValueError("PPO.guidance.coef_schedule: final_step=%d must be greater than initial_step=%d" % (out["final_step"], out["initial_step"]))
    return out


def schedule_coef(s, k):
    """The coefficient of update count k under a parse_schedule() dict as hgym_guide_schedule writes it, bit for bit: python doubles,
    left to right, rounded to fp32 once."""
    k = int(k)
    if s["mode"] == "step":
        v = s["coef"] if k < s["final_step"] else s["final_value"]
    elif s["mode"] == "linear":
        if k <= s["initial_step"]:
            v = s["coef"]
        elif k >= s["final_step"]:
            v = s["final_value"]
        else:
            v = s["coef"] + (s["final_value"] - s["coef"]) * float(k - s["initial_step"]) / float(s["final_step"] - s["initial_step"])
    else:
        v = s["coef"]
    return struct.unpack("f", struct.pack("f", v))[0]


def schedule_is_zero(s):
    """0 at every update count: the option is off."""
    return s["coef"] == 0.0 and s["final_value"] == 0.0


def run_out_step(s):
    """The first update count from which the coefficient is 0 for good, or None when there is none (then the term stays in the update)."""
    if schedule_is_zero(s):
        return 0
    return s["final_step"] if (s["mode"] != "constant" and s["final_value"] == 0.0) else None


def parse_config(cfg):
    """PPO.guidance -> None (off) or dict(teacher, schedule (parse_schedule), teacher_hidden_dims (list or None), teacher_activation,
    teacher_max_batch (int or None)).  ValueError: not a dict, an unknown key (named), a bad number (named)."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("PPO.guidance=%r: None or a dict is needed" % (cfg,))
    unknown = [k for k in cfg if k not in DEFAULTS]
    if unknown:
        raise ValueError("PPO.guidance: unknown key %s (known: %s)" % (", ".join(map(str, unknown)), ", ".join(DEFAULTS)))
    c = dict(DEFAULTS, **cfg)
    sched = parse_schedule(c["coef"], c["coef_schedule"])
    hd = c["teacher_hidden_dims"]
    if hd is not None:
        if not isinstance(hd, (list, tuple)) or not hd or any(isinstance(d, bool) or not isinstance(d, int) or d < 1 for d in hd):
            raise ValueError("PPO.guidance.teacher_hidden_dims=%r: a non-empty list of positive widths" % (hd,))
        hd = [int(d) for d in hd]
    mb = c["teacher_max_batch"]
    if mb is not None:
        if isinstance(mb, bool) or not isinstance(mb, int) or mb < 1:
            raise ValueError("PPO.guidance.teacher_max_batch=%r: a positive row count" % (mb,))
    act = c["teacher_activation"]
    if isinstance(act, str):
        if not hasattr(torch.nn, act):
            raise ValueError("PPO.guidance.teacher_activation=%r: no such torch.nn module" % (act,))
        act = getattr(torch.nn, act)()
    elif act is not None and not isinstance(act, torch.nn.Module):
        raise ValueError("PPO.guidance.teacher_activation=%r: a torch.nn module or its name" % (act,))
    if schedule_is_zero(sched):
        return None
    return dict(teacher=c["teacher"], schedule=sched, teacher_hidden_dims=hd, teacher_activation=act, teacher_max_batch=mb)


def check_setup(world=1, symmetry=None, mirror_loss_coef=0.0, smoothness=False, distillation=False):
    """What init_storage refuses with the option on (ValueError each; DESIGN.md section 33 names each as a follow-up): more than one rank;
    PPO.symmetry in either form and the mirror loss (separate heads; the mirrored half has no teacher column); PPO.smoothness (separate
    heads); Distillation."""
    if int(world) > 1:
        raise ValueError("PPO.guidance runs on one rank (world size %d)" % int(world))
    if symmetry is not None or float(mirror_loss_coef) > 0.0:
        raise ValueError("PPO.guidance does not support PPO.symmetry (augmentation or mirror loss): the mirrored rows have no teacher column")
    if smoothness:
        raise ValueError("PPO.guidance does not support PPO.smoothness: the two terms live in separate actor heads")
    if distillation:
        raise ValueError("PPO.guidance does not support Distillation: a cloning run has its own teacher")


# ------------------------------------------------------------------------------------------------ the teacher
def fold_obs_norm(W, b, mean, var, eps):
    """The first layer that takes RAW observations in place of normalised ones, (x - mean) / (sqrt(var) + eps): (W o s, b - (W o s) mean)
    with s = 1 / (sqrt(var) + eps), formed in float64 and rounded to fp32 once -- the fold export_policy_as_jit writes."""
    W64, b64 = torch.as_tensor(W).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    m64, v64 = torch.as_tensor(mean).detach().cpu().double().flatten(), torch.as_tensor(var).detach().cpu().double().flatten()
    if m64.numel() != W64.shape[1] or v64.numel() != W64.shape[1]:
        raise ValueError("PPO.guidance.teacher: %s has %d columns, actor.0.weight %d" % (OBS_NORM_KEY, m64.numel(), W64.shape[1]))
    s = 1.0 / (torch.sqrt(v64) + float(eps))
    Ws = W64 * s[None, :]
    return Ws.float(), (b64 - (Ws * m64[None, :]).sum(dim=1)).float()


def teacher_tensors(teacher):
    """`teacher` as PPO.guidance takes it -> {"actor.<2l>.weight" / ".bias": fp32 cpu tensor}, the statistics of a teacher trained with
    empirical_normalization folded into the first layer (fold_obs_norm).  ValueError for anything with no `actor.*` entries."""
    norm = None
    if isinstance(teacher, (str, os.PathLike)):
        teacher = torch.load(teacher, map_location="cpu")
    if isinstance(teacher, torch.nn.Module):
        if hasattr(teacher, "norm_state_dicts"):
            norm = teacher.norm_state_dicts().get(OBS_NORM_KEY)
        sd = teacher.state_dict()
        if not any(k.startswith("actor.") for k in sd):      # the actor itself (a Sequential)
            sd = {"actor." + k: v for k, v in sd.items()}
    elif isinstance(teacher, dict):
        if "model_state_dict" in teacher:
            norm, sd = teacher.get(OBS_NORM_KEY), teacher["model_state_dict"]
        else:
            sd = teacher
    else:
        raise ValueError("PPO.guidance.teacher=%r: a checkpoint path, a state dict or a module is needed" % (type(teacher).__name__,))
    out = {k: torch.as_tensor(v).detach().cpu().float().clone() for k, v in sd.items() if k.startswith("actor.") and k.endswith((".weight", ".bias"))}
    if "actor.0.weight" not in out:
        raise ValueError("PPO.guidance.teacher has no `actor.0.weight`: a PPO checkpoint (or its model_state_dict) is needed")
    if norm is not None:
        out["actor.0.weight"], out["actor.0.bias"] = fold_obs_norm(out["actor.0.weight"], out["actor.0.bias"], norm["mean"], norm["var"], norm["eps"])
    return out


def teacher_dims(tensors):
    """(input width, hidden widths, output width) from the shapes of the actor.<2l>.weight entries, checked to chain."""
    n = 0
    while "actor.%d.weight" % (2 * n) in tensors:
        n += 1
    shapes = [tuple(tensors["actor.%d.weight" % (2 * l)].shape) for l in range(n)]
    for l in range(n):
        if len(shapes[l]) != 2 or (l and shapes[l][1] != shapes[l - 1][0]) or tuple(tensors.get("actor.%d.bias" % (2 * l), torch.empty(0)).shape) != (shapes[l][0],):
            raise ValueError("PPO.guidance.teacher: actor.%d.weight / .bias do not chain (shapes %s)" % (2 * l, shapes))
    if n < 2:
        raise ValueError("PPO.guidance.teacher: at least one hidden layer is needed (found %d linear layers)" % n)
    return shapes[0][1], [s[0] for s in shapes[:-1]], shapes[-1][0]


def check_teacher(tensors, num_actor_obs, num_actions, hidden_dims=None):
    """The teacher's widths against the student's, by name; -> its hidden widths."""
    n_in, hidden, n_out = teacher_dims(tensors)
    if n_in != int(num_actor_obs):
        raise ValueError("PPO.guidance.teacher: actor.0.weight takes %d inputs, the student's num_actor_obs is %d" % (n_in, int(num_actor_obs)))
    if n_out != int(num_actions):
        raise ValueError("PPO.guidance.teacher: actor.%d.weight has %d outputs, num_actions is %d" % (2 * len(hidden), n_out, int(num_actions)))
    if hidden_dims is not None and list(hidden_dims) != hidden:
        raise ValueError("PPO.guidance.teacher_hidden_dims=%r, the teacher's actor.* weights have %r" % (list(hidden_dims), hidden))
    return hidden


def check_state_dict(sd, name, on, schedule=None):
    """A checkpoint with STATE_KEY for a run without the option, the reverse, or one saved under another schedule: refused by key name."""
    if sd is not None and not on:
        raise RuntimeError("%s carries `%s`: it was trained with PPO.guidance, this run was built without it" % (name, STATE_KEY))
    if sd is None and on:
        raise RuntimeError("%s has no `%s`: it was trained without PPO.guidance, this run was built with it" % (name, STATE_KEY))
    if sd is not None and dict(sd["schedule"]) != dict(schedule):
        raise RuntimeError("%s: `%s` was saved with the schedule %r; this run was built with %r" % (name, STATE_KEY, dict(sd["schedule"]), dict(schedule)))


# ------------------------------------------------------------------------------------------------ the option's device side
class Guidance:
    """The option as PPO holds it (PPO._guide; None: off).  `count`: the number of updates completed (the host's; `count_dev` is what
    hgym_guide_schedule reads and advances).  `active`: the schedule has not run out -- once it has, compute_returns and update() leave the
    option's launches out and the graph key says so."""

    def __init__(self, cfg, actor_critic, net, rows, device):
        """cfg: parse_config()'s dict.  The teacher in a forward-only NetBuffers of its own, built the way StudentTeacher.bind builds its
        own: the student's precision, a placeholder critic, max_batch capped at TEACHER_MAX_BATCH.  rows: T N, the stored rows the
        teacher's pass covers.  Everything is allocated here, nothing during an iteration."""
        import hgym
        self._hgym = hgym
        self.cfg, self.schedule, self.device = cfg, cfg["schedule"], device
        self.num_obs, self.num_actions, self.rows = int(actor_critic.num_actor_obs), int(actor_critic.num_actions), int(rows)
        self.tensors = None if cfg["teacher"] is None else teacher_tensors(cfg["teacher"])
        if self.tensors is None and cfg["teacher_hidden_dims"] is None:
            raise ValueError("PPO.guidance.teacher is None: teacher_hidden_dims is needed to build the teacher a checkpoint will fill (load)")
        self.hidden = cfg["teacher_hidden_dims"] if self.tensors is None else check_teacher(self.tensors, self.num_obs, self.num_actions,
                                                                                            cfg["teacher_hidden_dims"])
        self.activation = cfg["teacher_activation"] if cfg["teacher_activation"] is not None else getattr(actor_critic, "activation", None)
        mb = int(cfg["teacher_max_batch"]) if cfg["teacher_max_batch"] else min(int(net.cfg.max_batch), TEACHER_MAX_BATCH)
        tcfg = hgym.make_net_config(self.num_obs, int(actor_critic.num_critic_obs), self.num_actions, self.hidden, PLACEHOLDER_CRITIC_DIMS,
                                    int(net.cfg.precision), mb, activation=self.activation,
                                    fused_activation=getattr(actor_critic, "fused_activation", False),
                                    noise_std_type=getattr(actor_critic, "noise_std_type", "scalar"))
        self.tnet = hgym.NetBuffers(tcfg, device)
        self.tnet.params[:self.num_actions] = 1.0 if getattr(actor_critic, "noise_std_type", "scalar") != "log" else 0.0      # a valid sigma; nothing reads it
        self.loaded = False
        if self.tensors is not None:
            self._load_teacher(self.tensors)
        z = lambda n, dtype: torch.zeros(n, dtype=dtype, device=device)
        self.count, self.count_dev, self.coef = 0, z(1, torch.int64), z(1, torch.float32)
        self.block = z(3, torch.float64)      # [0] the sum of the minibatches' MSEs, [1] their number, [2] the coefficient as the log reads it
        self.sums = self.block[0:2]
        self.struct = hgym.make_guide_schedule(self.schedule["mode"], self.schedule["coef"], self.schedule["final_value"],
                                               self.schedule["initial_step"], self.schedule["final_step"])
        self._retired, self._out = False, run_out_step(self.schedule)
        self.last, self.teacher_mu = None, None

    def _load_teacher(self, tensors):
        with torch.no_grad():
            for k, v in tensors.items():
                self.tnet.views[k].copy_(v.to(self.tnet.views[k].device))
        self.tnet.sync_shadow()
        self.tensors, self.loaded = {k: v.detach().cpu().float().clone() for k, v in tensors.items()}, True

    @property
    def active(self):
        return self._out is None or self.count < self._out

    def bind_storage(self, storage):
        self.teacher_mu = storage.teacher_mu.view(-1, self.num_actions)
        assert self.teacher_mu.data_ptr() % 16 == 0

    def teacher_pass(self, storage):
        """The end of compute_returns: the teacher's mean of all T N stored observation rows, in pieces, into storage.teacher_mu."""
        if not self.loaded:
            raise RuntimeError("PPO.guidance: the teacher is not loaded (PPO.guidance[\"teacher\"] is None and no checkpoint with `%s` was loaded)" % STATE_KEY)
        T = storage.num_transitions_per_env
        forward_in_pieces(self.tnet, storage._obs_all[:T].flatten(0, 1), self.teacher_mu[:self.rows])

    def begin_update(self):
        """The start of update(): this update's coefficient on the device and the count advanced (one launch with fixed arguments), the two
        sums zeroed, the coefficient into the log's double.  Eager calls re-seat the device count from the host's first (what a resume
        set); under capture nothing is re-seated -- replays continue the device count."""
        with torch.inference_mode():
            if not torch.cuda.is_current_stream_capturing():
                self.count_dev.fill_(self.count)
            self._hgym.guide_schedule(self.struct, self.count_dev, self.coef)
            self.block[0:2] = 0.0      # (a slice: a fill kernel)
            self.block[2:3].copy_(self.coef)

    def minibatch(self):
        return self._hgym.make_guide(self.teacher_mu, self.coef, self.sums)

    def update_done(self):
        self.count += 1

    def retire_if_run_out(self):
        """Once, outside any capture, when the schedule has run out: the log's three numbers to 0, so that the log lines of the unguided
        rest of the run read 0 without any launch of the option in the update."""
        if not self.active and not self._retired and not torch.cuda.is_current_stream_capturing():
            with torch.inference_mode():
                self.block[0:3] = 0.0
                self.coef[0:1] = 0.0
            self._retired = True

    def graph_key(self):
        """PPO.update_graph_key's entry: the schedule's bytes and the buffers' addresses while the term is in the update, ("run out",) after."""
        if not self.active:
            return dict(guidance=("run out",))
        import ctypes as C
        return dict(guidance=(bytes(C.string_at(C.addressof(self.struct), C.sizeof(self.struct))), self.count_dev.data_ptr(), self.coef.data_ptr(),
                              self.block.data_ptr(), self.teacher_mu.data_ptr(), id(self.tnet)))

    def log_parts(self):
        return [("guide", self.block[0:2]), ("guide_coef", self.block[2:3])]

    def read_log(self, parts):
        """`last` = {loss, coef} from the parts of a host copy of PPO.log_block(): the mean unweighted MSE per minibatch and the coefficient."""
        s, n = (float(x) for x in parts["guide"])
        self.last = dict(loss=s / max(n, 1.0), coef=float(parts["guide_coef"][0]))
        return self.last

    def log_scalars(self):
        return [] if self.last is None else [("Loss/guidance", self.last["loss"]), ("Guidance/coef", self.last["coef"])]

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """Host data only (nothing is read from the device): the count, the parsed schedule and the teacher's actor tensors as they were
        loaded (statistics folded), so that a resume needs no teacher file."""
        return dict(count=int(self.count), schedule=dict(self.schedule), teacher={k: v.clone() for k, v in (self.tensors or {}).items()},
                    teacher_hidden_dims=list(self.hidden))

    def load_state_dict(self, sd):
        tensors = {k: torch.as_tensor(v).detach().cpu().float() for k, v in sd["teacher"].items()}
        check_teacher(tensors, self.num_obs, self.num_actions, self.hidden)
        self._load_teacher(tensors)
        self.count = int(sd["count"])
        with torch.inference_mode():
            self.count_dev.fill_(self.count)
        self._retired = False
        self.retire_if_run_out()
