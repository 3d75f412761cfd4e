"""Checkpoint files of OnPolicyRunner: what model_<it>.pt and its sidecar envstate_<it>.pt contain, how they reach the disk and what
load() refuses (the runner's save() / load() hold the contract).  Two ways to the same file.  Blocking: the modules' own state_dict()
calls plus extra_entries(), written on the training thread.  Background, the device path (background_eligible): the tensors are first
copied to pinned host memory stream-side (Snapshot.take: behind whatever the update has enqueued -- the host does not wait) and cut
into the same dict (assemble), pickled + written by a background thread, so a checkpoint costs the training thread ~0.1 ms instead of a
device sync + 5-15 ms (round 6: default; `test_background_checkpoint_equals_the_synchronous_one`).  HGYM_ASYNC_SAVE=0 restores the
reference's blocking torch.save everywhere.  write_atomic() is the only place that writes a file."""
import atexit
import os
import queue
import sys
import threading
import time

import torch

NORM_KEYS = ("obs_norm_state_dict", "critic_obs_norm_state_dict")      # a checkpoint of a run with empirical_normalization carries both
RND_STATE_KEY = "rnd_state_dict"      # what a checkpoint of a run with rnd_cfg carries besides the reference's four keys
VALUE_NORM_KEY = "value_norm_state_dict"      # what a checkpoint of a run with PPO.value_normalization carries: count, mean, var, eps
GUIDE_KEY = "guidance_state_dict"      # what a checkpoint of a run with PPO.guidance carries: count, schedule, the teacher's actor tensors
WARMUP_KEY = "critic_warmup_state_dict"      # what a checkpoint of a run with PPO.critic_warmup_updates > 0 carries: done, updates
NORM_COUNT = 2      # NetBuffers.norm_view("header"): eps, until, then count of statistics k at NORM_COUNT + k, of L.NORM_HEADER_DOUBLES doubles


class _CheckpointWriter:
    """One background thread that turns pinned-host snapshots into checkpoint files (OnPolicyRunner.save): the training thread only
    enqueues device -> pinned-host copies behind the update and goes on; the pickling + file write (6-15 ms for XBot-L's 11 MB of
    parameters and Adam moments) happens here, under the next iteration.  Files appear atomically (written to a temporary name,
    then renamed)."""

    def __init__(self):
        self.q = queue.Queue()
        self.thread = None
        self.error = None
        self.lock = threading.Lock()

    def submit(self, job):
        with self.lock:
            if self.thread is None or not self.thread.is_alive():
                self.thread = threading.Thread(target=self._run, name="hgym-checkpoint-writer", daemon=True)
                self.thread.start()
        self.q.put(job)

    def _run(self):
        # this thread's CPU tensor work stays on this thread: the default intra-op pool is one thread per host core (128+ on the GPU boxes), and a
        # parallel region opened from here -- a 3.7 MB copy is enough -- wakes all of them next to the thread that launches the kernels
        # (measured: sporadic 50-350 ms stalls of a checkpoint job and, now and then, of the training thread; profiles/r06_async_checkpoint_default.txt)
        try:
            torch.set_num_threads(1)
        except Exception:      # noqa: BLE001
            pass
        while True:
            job = self.q.get()
            try:
                if job is not None:
                    job()
            except Exception as e:      # noqa: BLE001 -- re-raised on the training thread by wait()
                self.error = e
            finally:
                self.q.task_done()

    def wait(self):
        self.q.join()
        if self.error is not None:
            e, self.error = self.error, None
            raise e


WRITER = _CheckpointWriter()
atexit.register(lambda: WRITER.q.join())


def env_state_path(path):
    """The sidecar that goes with checkpoint `path`: envstate_<it>.pt next to model_<it>.pt.  Its name never contains "model":
    helpers.get_load_path takes the last file of a run directory whose name does."""
    d, base = os.path.split(path)
    return os.path.join(d, "envstate" + base[len("model"):] if base.startswith("model") else "envstate_" + base.replace("model", "ckpt"))


def write_atomic(obj, path):
    """torch.save under a temporary name (the pid in it), then renamed: `path` is either absent or complete."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    torch.save(obj, tmp)
    os.replace(tmp, path)


def write_checkpoint(ck, path, side=None):
    """The sidecar (when there is one) is renamed into place BEFORE the model file, so a visible model_<it>.pt has its sidecar."""
    if side is not None:
        write_atomic(side, env_state_path(path))
    write_atomic(ck, path)


# ------------------------------------------------------------------ what a checkpoint contains
def extra_entries(alg):
    """What a checkpoint carries beyond the reference's four keys, in file order: the two normaliser dicts (NORM_KEYS) of a policy with
    empirical_normalization, then RND_STATE_KEY of a run with rnd_cfg, then VALUE_NORM_KEY of a run with PPO.value_normalization, then
    GUIDE_KEY of a run with PPO.guidance, then WARMUP_KEY of a run with PPO.critic_warmup_updates (both host data: the background path adds
    the same dicts).  Reads the device (the blocking path)."""
    ac, rnd = alg.actor_critic, alg._rnd
    extra = dict(ac.norm_state_dicts()) if hasattr(ac, "norm_state_dicts") else {}
    if rnd is not None:
        extra[RND_STATE_KEY] = rnd.rnd_state_dict()
    if getattr(alg, "value_normalizer", None) is not None:
        extra[VALUE_NORM_KEY] = alg.value_normalizer.state_dict()
    if getattr(alg, "_guide", None) is not None:
        extra[GUIDE_KEY] = alg._guide.state_dict()
    if getattr(alg, "_warmup", None) is not None:
        extra[WARMUP_KEY] = alg._warmup.state_dict()
    return extra


def sidecar_entries(alg, buf=None):
    """What the exact-resume sidecar carries beside the env's state and the run's counters: the AR(1) state of PPO.exploration_noise under
    exploration_noise.SIDECAR_KEY (a filter without a carried state, or the option off: nothing).  model_<it>.pt never changes with the
    option, so any checkpoint loads under any noise setting.  buf: the background path's snapshot buffer set (Snapshot.next_set) -- the
    state is copied stream-ordered into a pinned member of it, made on first use like the set's "norm" and "env" members."""
    from .exploration_noise import SIDECAR_KEY
    noise = getattr(alg, "_noise", None)
    if noise is None or noise.state is None:
        return {}
    out = None
    if buf is not None:
        if "noise" not in buf:
            buf["noise"] = torch.empty(noise.state.shape, dtype=torch.float32).pin_memory()
        out = buf["noise"]
    sd = noise.state_dict(out=out)
    return {} if sd is None else {SIDECAR_KEY: sd}


def load_sidecar_entries(side, alg):
    """sidecar_entries() of a loaded sidecar back into `alg`; an entry this run has no use for is ignored, a missing one leaves the state as built."""
    from .exploration_noise import SIDECAR_KEY
    if getattr(alg, "_noise", None) is not None:
        alg._noise.load_state_dict(side.get(SIDECAR_KEY))


def param_layout(state_dict, params):
    """[(name, offset, shape)] of every state_dict entry in the flat vector `params`: state_dict order = nn.Module's named_parameters
    order.  Every entry must be an fp32 view INTO the flat vector (assemble cuts by offset and shape only)."""
    base, layout = params.data_ptr(), []
    for k, v in state_dict.items():
        o = (v.data_ptr() - base) // 4
        assert v.dtype == torch.float32 and v.is_contiguous(), "%s is not an fp32 view of the flat parameter vector" % k
        assert 0 <= o and o + v.numel() <= params.numel() and (v.data_ptr() - base) % 4 == 0, "%s lies outside the flat parameter vector" % k
        layout.append((k, o, tuple(v.shape)))
    return layout


def assemble(buf, layout, opt_layout, group, it, infos, norm=None, value_norm=None):
    """The checkpoint dict from a host snapshot, key for key what the blocking path saves.  buf: flat `params`, `m`, `v` (fp32) and `opt`
    (opt_state), and with norm = ((num_obs, num_priv), (eps, until)) also `norm`: the header, then mean / var of both statistics (fp64).
    value_norm = eps: `value_norm` holds the three doubles (count, mean, var) -> VALUE_NORM_KEY, python floats as the blocking path's.
    layout: param_layout(); opt_layout: [(offset, shape)] of the optimiser's views; group: the hyper-parameters without lr and params.
    The tensors are views INTO the snapshot, no copies: torch.save writes each flat buffer once (tensors that share a storage are
    pickled as offset + shape into it), torch.load hands back the same named tensors."""
    from hgym import _lib as L
    cut = lambda t, o, shp: t[o:o + int(torch.Size(shp).numel())].view(shp)
    # (alg.optimizer.param_groups reads the learning rate from the device: a host sync; the snapshot carries it instead)
    lr, step = float(buf["opt"][L.OPT_LR]), float(buf["opt"][L.OPT_STEP])
    state = {i: dict(step=torch.tensor(step), exp_avg=cut(buf["m"], o, shp), exp_avg_sq=cut(buf["v"], o, shp))
             for i, (o, shp) in enumerate(opt_layout)}
    ck = {"model_state_dict": {k: cut(buf["params"], o, shp) for k, o, shp in layout},
          "optimizer_state_dict": dict(state=state, param_groups=[dict(lr=lr, **group, params=list(range(len(state))))]),
          "iter": it, "infos": infos}
    if norm is not None:
        (K, (eps, until)), nb, o = norm, buf["norm"], L.NORM_HEADER_DOUBLES
        for k, key in enumerate(NORM_KEYS):
            ck[key] = dict(mean=nb[o:o + K[k]].clone(), var=nb[o + K[k]:o + 2 * K[k]].clone(), count=float(nb[NORM_COUNT + k]), eps=eps, until=until)
            o += 2 * K[k]
    if value_norm is not None:
        count, mean, var = (float(x) for x in buf["value_norm"])
        ck[VALUE_NORM_KEY] = dict(count=count, mean=mean, var=var, eps=float(value_norm))
    return ck


def background_eligible(alg, device):
    """Does save() take the background path?  A device run with the fused network bound (alg.net, actor_critic._net), unless
    HGYM_ASYNC_SAVE=0 restores the reference's blocking torch.save everywhere.  Not a StudentTeacher: its teacher.* entries live in a
    second flat vector, and the blocking form cuts nothing by offset.  Not with RND: its two nets, the predictor's optimiser and the
    reward pass's block live in buffers of their own."""
    return (getattr(alg, "net", None) is not None and str(device).startswith("cuda") and os.environ.get("HGYM_ASYNC_SAVE", "1") != "0"
            and hasattr(alg.actor_critic, "_net") and getattr(alg.actor_critic, "_teacher_net", None) is None
            and alg._rnd is None)


class Snapshot:
    """Two alternating sets of pinned host buffers (two snapshots in flight at most: the writer is two checkpoints behind only if the
    disk is).  A set's `busy` event is set while the set is free; its "norm" and "env" members are pinned on first use, so a run
    without normalisation or without exact_resume allocates nothing for them."""

    def __init__(self, net):
        mk = lambda n, dt: torch.empty(n, dtype=dt).pin_memory()
        self.sets = [dict(params=mk(net.P, torch.float32), m=mk(net.P, torch.float32), v=mk(net.P, torch.float32),
                          opt=mk(net.opt_state.numel(), net.opt_state.dtype), busy=threading.Event()) for _ in range(2)]
        for b in self.sets:
            b["busy"].set()
        self.n = 0

    def next_set(self):
        """The buffer set the next take() fills, once it is free: for a caller that enqueues a copy of its own into a member of the set
        ahead of take()'s event (checkpoint.sidecar_entries)."""
        buf = self.sets[self.n & 1]
        buf["busy"].wait()
        return buf

    def take(self, net, actor_critic, env=None, value_norm=None):
        """Enqueue the device -> pinned copies of one checkpoint (env: its state too) -> what write_snapshot needs: the buffer set, the event
        behind the copies, the layouts (recomputed per save), the normaliser's shape (None: off) and the env's snapshot (None: not asked)."""
        buf = self.sets[self.n & 1]
        self.n += 1
        buf["busy"].wait()
        buf["busy"].clear()
        for name, src in (("params", net.params), ("m", net.adam_m), ("v", net.adam_v), ("opt", net.opt_state)):
            buf[name].copy_(src, non_blocking=True)
        norm = None
        if getattr(net, "obs_norm", None) is not None:       # the normaliser's state rides with the parameters, in assemble()'s order
            parts = [net.norm_view("header")] + [net.norm_view(n, k) for k in (0, 1) for n in ("mean", "var")]
            if "norm" not in buf:
                buf["norm"] = torch.empty(sum(t.numel() for t in parts), dtype=torch.float64).pin_memory()
            o = 0
            for t in parts:
                buf["norm"][o:o + t.numel()].copy_(t, non_blocking=True)
                o += t.numel()
            norm = ((int(net.cfg.num_obs), int(net.cfg.num_priv)), net.obs_norm)
        if value_norm is not None:      # (block, eps) of PPO.value_normalization: three doubles ride with the parameters
            if "value_norm" not in buf:
                buf["value_norm"] = torch.empty(3, dtype=torch.float64).pin_memory()
            buf["value_norm"].copy_(value_norm[0], non_blocking=True)
        env_state = None
        if env is not None:
            if "env" not in buf:
                buf["env"] = env.state_host_buffers()
            env_state = env.state_dict(out=buf["env"])
        done = torch.cuda.Event()
        done.record()
        return dict(buf=buf, done=done, layout=param_layout(actor_critic.state_dict(), net.params), norm=norm, env=env_state,
                    value_norm=None if value_norm is None else float(value_norm[1]),
                    opt_layout=[(o, shape) for _, o, shape in param_layout(net.views, net.params)])


def write_snapshot(shot, group, it, infos, path, side):
    """The writer's job for one Snapshot.take(): waits for the copies' event, never for the device; frees the buffer set at the end."""
    try:
        tj = [time.perf_counter()]
        shot["done"].synchronize()
        tj.append(time.perf_counter())
        ck = assemble(shot["buf"], shot["layout"], shot["opt_layout"], group, it, infos, shot["norm"], shot.get("value_norm"))
        if shot.get("guidance") is not None:      # PPO.guidance: Guidance.state_dict() as the training thread formed it at save() (host data)
            ck[GUIDE_KEY] = shot["guidance"]
        if shot.get("critic_warmup") is not None:      # PPO.critic_warmup_updates: the count as it stood at save() (host data)
            ck[WARMUP_KEY] = shot["critic_warmup"]
        tj.append(time.perf_counter())
        write_checkpoint(ck, path, side)
        tj.append(time.perf_counter())
        if os.environ.get("HGYM_SAVE_TRACE"):
            sys.stderr.write("writer job %s: event %.2f, cut %.2f, torch.save + rename %.2f ms\n" % (
                os.path.basename(path), *[(b - a) * 1e3 for a, b in zip(tj, tj[1:])]))
    finally:
        shot["buf"]["busy"].set()


# ------------------------------------------------------------------ the sidecar's switches
def _data_parallel(holder, world_size, text):
    """Data-parallel runs: every rank's env is its own and only rank 0 writes checkpoints, so env state is neither saved nor loaded
    there -- said once per holder (the runner), and the run goes on as without the switch."""
    if world_size > 1 and not holder._warned_env_state:
        holder._warned_env_state = True
        print(text)
    return world_size > 1


def exact_resume_on(cfg, world_size, holder):
    """cfg["exact_resume"] (absent: off), on one rank."""
    return bool(cfg.get("exact_resume", False)) and not _data_parallel(
        holder, world_size, "exact_resume: env state is not saved in a data-parallel run (world size %d); checkpoints are written as without it" % world_size)


def resolve_sidecar(path, env_state, world_size, holder):
    """The sidecar load() reads with checkpoint `path`, or None.  env_state: None (the one beside `path` if it exists), False (none) or
    a path (that one, existing or not)."""
    if env_state is False:
        return None
    explicit = isinstance(env_state, (str, os.PathLike))
    side_path = env_state if explicit else env_state_path(path)
    if not explicit and not os.path.exists(side_path):
        return None
    if _data_parallel(holder, world_size, "exact_resume: %s is not loaded in a data-parallel run (world size %d); resuming as without it"
                      % (os.path.basename(side_path), world_size)):
        return None
    return side_path


def check_sidecar(side, num_steps_per_env, env, alg=None):
    """A sidecar that does not fit this run, this env or (alg) this run's exploration-noise state: refused before anything is changed."""
    if int(side["world_size"]) != 1:
        raise ValueError("env state: world_size is %d in the sidecar; exact resume covers one rank" % int(side["world_size"]))
    if int(side["num_steps_per_env"]) != int(num_steps_per_env):
        raise ValueError("env state: num_steps_per_env is %d in the sidecar, %d here" % (int(side["num_steps_per_env"]), num_steps_per_env))
    env.check_state_dict(side["env"])
    if getattr(alg, "_noise", None) is not None:
        from .exploration_noise import SIDECAR_KEY
        alg._noise.check_state_dict(side.get(SIDECAR_KEY))


# ------------------------------------------------------------------ what load() refuses
def _check_norm_keys(loaded, has_norm, name, spec=None):
    """A checkpoint with statistics for a policy built without normalisation, or the reverse: refused, naming the key.  spec: this policy's
    (eps, until) -- statistics saved under another eps or until are another function of the observations, or stop elsewhere: refused too."""
    for k in NORM_KEYS:
        if (k in loaded) != has_norm:
            if has_norm:
                raise RuntimeError("%s has no `%s`: it was trained without empirical_normalization, this policy was built with it" % (name, k))
            raise RuntimeError("%s carries `%s`: it was trained with empirical_normalization, this policy was built without it" % (name, k))
        if has_norm and spec is not None:
            theirs = (loaded[k].get("eps"), loaded[k].get("until"))
            if theirs[0] is None or float(theirs[0]) != float(spec[0]) or theirs[1] != spec[1]:
                raise RuntimeError("%s: `%s` was saved with normalization_eps=%r, normalization_until=%r; this policy was built with %r, %r"
                                   % (name, k, theirs[0], theirs[1], spec[0], spec[1]))


def value_norm_spec(alg):
    """check_compatible's value_norm argument for `alg`: the option's eps, or None when PPO.value_normalization is off."""
    vn = getattr(alg, "value_normalizer", None)
    return None if vn is None else vn.eps


def _check_value_norm_key(loaded, eps, name):
    """A checkpoint of a run with PPO.value_normalization for a run without it, or the reverse, or one saved under another eps: the critic's
    parameters mean another function of the state under the same names.  Refused by key name."""
    sd = loaded.get(VALUE_NORM_KEY)
    if sd is not None and eps is None:
        raise RuntimeError("%s carries `%s`: it was trained with PPO.value_normalization (its critic outputs normalised values), this run "
                           "was built without it" % (name, VALUE_NORM_KEY))
    if sd is None and eps is not None:
        raise RuntimeError("%s has no `%s`: it was trained without PPO.value_normalization (its critic outputs raw values), this run was "
                           "built with it" % (name, VALUE_NORM_KEY))
    if sd is not None and (sd.get("eps") is None or float(sd["eps"]) != float(eps)):
        raise RuntimeError("%s: `%s` was saved with value_normalization_eps=%r; this run was built with %r" % (name, VALUE_NORM_KEY, sd.get("eps"), eps))


def check_compatible(loaded, actor_critic, rnd, name, value_norm=None, guidance=None, critic_warmup=False):
    """Checkpoint `loaded` (file `name`) against this run's policy, RND module (None: off), value normalisation (value_norm: its eps,
    None: off), guidance (the run's Guidance, None: off) and critic warm-up (on?); raises before anything is changed."""
    # a checkpoint of the other noise parametrisation: its first entry is another quantity under another name
    msd, mine = loaded["model_state_dict"], getattr(actor_critic, "noise_std_type", "scalar")
    theirs = "log" if "log_std" in msd else ("scalar" if "std" in msd else mine)
    if theirs != mine:
        raise RuntimeError("%s was trained with noise_std_type=\"%s\" (its model_state_dict has `%s`); this policy was built with "
                           "noise_std_type=\"%s\"" % (name, theirs, "log_std" if theirs == "log" else "std", mine))
    # a checkpoint with the normaliser's statistics for a policy without normalisation, or the reverse: another function of the
    # observations under the same parameter names
    _check_norm_keys(loaded, bool(getattr(actor_critic, "empirical_normalization", False)), name, getattr(actor_critic, "obs_norm_spec", None))
    # a checkpoint of a run with RND for a run without it, or the reverse, or the per-env average of another number of envs: refused by name
    from .rnd import check_state_dict as check_rnd_state
    check_rnd_state(loaded.get(RND_STATE_KEY), name, rnd is not None, getattr(rnd, "num_envs", None))
    _check_value_norm_key(loaded, value_norm, name)
    # a checkpoint of a guided run for a run without the option, the reverse, or another schedule: refused by key name
    from .guidance import check_state_dict as check_guide_state
    check_guide_state(loaded.get(GUIDE_KEY), name, guidance is not None, getattr(guidance, "schedule", None))
    # a checkpoint of a run with critic warm-up for a run without it, or the reverse: refused by key name
    from .critic_warmup import check_state_dict as check_warmup_state
    check_warmup_state(loaded.get(WARMUP_KEY), name, bool(critic_warmup))
