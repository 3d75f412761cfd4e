"""The smoothness regulariser on the policy's mean (PPO.smoothness): the configuration and what init_storage refuses,
as functions that need no device, and the option's device side, Smoothness.

PPO.smoothness = None | dict with the keys of DEFAULTS:
  temporal_coef  lamT >= 0: pulls mu(s_t) towards mu(s_t+1) (rows whose episode ended weigh 0)
  spatial_coef   lamS >= 0: pulls mu(s) towards mu(s + noise_std * z)
  noise_std      a scalar or a (num_obs,) vector, raw observation units; needed with spatial_coef > 0 (OnPolicyRunner fills it with the env's
                 noise_scale_vec * noise_level tiled over the stacked frames)
  noise_scale    a factor on noise_std (default 1.0)
  seed           the Philox key of the perturbation (default: the run's seed)
None, or both coefficients 0: off."""
import math

import torch

DEFAULTS = dict(temporal_coef=0.0, spatial_coef=0.0, noise_std=None, noise_scale=1.0, seed=None)


def parse_config(cfg, num_obs, default_seed=0):
    """PPO.smoothness -> None (off) or dict(temporal_coef, spatial_coef, noise_std (a list of num_obs floats, or None with the spatial term
    off), seed).  ValueError: not a dict, an unknown key (named), a coefficient or a noise that is negative or not finite, a noise_std
    vector of another length, spatial_coef > 0 without noise_std."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("PPO.smoothness=%r: None or a dict is needed" % (cfg,))
    unknown = [k for k in cfg if k not in DEFAULTS]
    if unknown:
        raise ValueError("PPO.smoothness: unknown key %s (known: %s)" % (", ".join(map(str, unknown)), ", ".join(DEFAULTS)))
    c = dict(DEFAULTS, **cfg)
    out = {}
    for k in ("temporal_coef", "spatial_coef", "noise_scale"):
        try:
            v = float(c[k])
        except (TypeError, ValueError):
            raise ValueError("PPO.smoothness.%s=%r: a number is needed" % (k, c[k]))
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError("PPO.smoothness.%s=%r: must be finite and >= 0" % (k, c[k]))
        out[k] = v
    if out["temporal_coef"] == 0.0 and out["spatial_coef"] == 0.0:
        return None
    ns = c["noise_std"]
    if ns is None:
        if out["spatial_coef"] > 0.0:
            raise ValueError("PPO.smoothness.spatial_coef=%r needs noise_std (a scalar or %d values)" % (c["spatial_coef"], int(num_obs)))
    else:
        if hasattr(ns, "tolist"):
            ns = ns.tolist()
        vals = [float(x) for x in ns] if isinstance(ns, (list, tuple)) else [float(ns)] * int(num_obs)
        if len(vals) != int(num_obs):
            raise ValueError("PPO.smoothness.noise_std has %d values, the observation %d" % (len(vals), int(num_obs)))
        if not all(v >= 0.0 and math.isfinite(v) for v in vals):
            raise ValueError("PPO.smoothness.noise_std: every value must be finite and >= 0")
        ns = [v * out["noise_scale"] for v in vals]
    seed = default_seed if c["seed"] is None else c["seed"]
    return dict(temporal_coef=out["temporal_coef"], spatial_coef=out["spatial_coef"], noise_std=ns, seed=int(seed) & 0xFFFFFFFFFFFFFFFF)


def check_setup(world=1, symmetry=None, distillation=False):
    """What init_storage refuses with the regulariser on (ValueError each; DESIGN.md section 28 names each as a follow-up): more than one
    rank; a `symmetry` that is not None (the mirrored half stores no mirrored bootstrap slot); Distillation.  PPO.check_setup withholds its
    MirrorSpec exactly when the mirror loss is on without augmentation: that form combines."""
    if int(world) > 1:
        raise ValueError("PPO.smoothness runs on one rank (world size %d)" % int(world))
    if symmetry is not None:
        raise ValueError("PPO.smoothness does not support PPO.symmetry (augmentation or mirror loss)")
    if distillation:
        raise ValueError("PPO.smoothness does not support Distillation")


class Smoothness:
    """The option as PPO holds it (PPO._smooth; None: off): the parse_config() dict `cfg`, everything hgym_smooth_pairs and
    hgym_ppo_grad_smooth name, and its part of the log.  `head_partials`: hgym_ppo_grad_smooth_mirror's scratch, None unless the mirror loss
    is on beside the regulariser."""
    BUFFERS = ("next_idx", "next_weight", "noise_std", "target_next", "target_near", "rows", "sums")

    def __init__(self, cfg, perm_len, mb, num_obs, num_actions, device, mirror_loss=False):
        """Allocated once (torch.zeros: nothing is allocated during an update) -- next_idx / next_weight for a whole permutation of
        perm_len rows, noise_std (num_obs; zeros when the spatial term is off), and for one minibatch of mb rows target_next, target_near
        (mb x num_actions) and rows (mb x the width rounded up to 4), then the four sums; mirror_loss: head_partials as well."""
        import hgym
        z = lambda n, dtype=torch.float32: torch.zeros(max(int(n), 1), dtype=dtype, device=device)
        self.cfg, self.mb, self.last = cfg, int(mb), None
        self.next_idx, self.next_weight, self.noise_std = z(perm_len, torch.int64), z(perm_len), z(num_obs)
        if cfg["noise_std"] is not None:
            self.noise_std.copy_(torch.tensor(cfg["noise_std"], dtype=torch.float32))
        self.target_next, self.target_near = z(mb * num_actions), z(mb * num_actions)
        self.rows, self.sums = z(mb * hgym.smooth_ld(num_obs)), z(4, torch.float64)
        self.head_partials = z(hgym.smooth_mirror_partials(mb)) if mirror_loss else None

    def begin_update(self, perm, storage):
        """One pass over the whole permutation: every epoch reuses the slices, as the advantage pass's are."""
        import hgym
        hgym.smooth_pairs(perm, storage.dones.view(-1), storage.num_envs, self.next_idx, self.next_weight)
        self.sums[0:4] = 0.0      # (a slice: a fill kernel)

    def minibatch(self, i):
        """hgym_ppo_grad_smooth's descriptor of minibatch i: its slices of the successor map, and no next_idx with the temporal term off."""
        import hgym
        c, rows = self.cfg, slice(i * self.mb, (i + 1) * self.mb)
        return hgym.make_smooth(c["temporal_coef"], c["spatial_coef"], next_idx=self.next_idx[rows] if c["temporal_coef"] > 0.0 else None,
                                next_weight=self.next_weight[rows], noise_std=self.noise_std, seed=c["seed"], target_next=self.target_next,
                                target_near=self.target_near, rows=self.rows, sums=self.sums)

    def graph_key(self):
        """PPO.update_graph_key's entry: the coefficients and the seed, and the scratch the launches name (head_partials last, when there)."""
        c = self.cfg
        hp = () if self.head_partials is None else (self.head_partials.data_ptr(),)
        return dict(smoothness=(c["temporal_coef"], c["spatial_coef"], c["seed"]) + tuple(getattr(self, n).data_ptr() for n in self.BUFFERS) + hp)

    def log_parts(self):
        return [("smooth", self.sums)]

    def read_log(self, parts):
        """`last` = {temporal, spatial, valid_fraction} from the parts of a host copy of PPO.log_block(): the mean plain MSE per minibatch
        of either term and the share of drawn rows with a successor."""
        t, s, w, n = (float(x) for x in parts["smooth"])
        n = max(n, 1.0)
        self.last = dict(temporal=t / n, spatial=s / n, valid_fraction=w / (self.mb * n))
        return self.last

    def log_scalars(self):
        return [] if self.last is None else [("Loss/smooth_temporal", self.last["temporal"]), ("Loss/smooth_spatial", self.last["spatial"])]


def env_noise_std(env_cfg, noise_scale_vec, num_obs):
    """The env's own sensor noise per stacked observation column: noise_scale_vec * cfg.noise.noise_level tiled over the frames (a list of
    num_obs floats), or None when the env states none."""
    noise = getattr(env_cfg, "noise", None)
    if noise_scale_vec is None or noise is None or getattr(noise, "noise_level", None) is None:
        return None
    frame = [float(x) * float(noise.noise_level) for x in (noise_scale_vec.tolist() if hasattr(noise_scale_vec, "tolist") else noise_scale_vec)]
    if not frame or int(num_obs) % len(frame) != 0:
        return None
    return frame * (int(num_obs) // len(frame))


def check_noise_mirror(noise_std, obs_src):
    """With the mirror loss beside the spatial term the perturbation must treat left and right alike, or it fights the mirror term:
    noise_std[obs_src[c]] == noise_std[c] for every observation column c (obs_src: the MirrorSpec's observation table, the column each
    mirrored column is read from).  ValueError naming the first column that breaks it.  The env's own noise_scale_vec passes."""
    ns = noise_std.tolist() if hasattr(noise_std, "tolist") else list(noise_std)
    src = obs_src.tolist() if hasattr(obs_src, "tolist") else list(obs_src)
    if len(ns) != len(src):
        raise ValueError("PPO.smoothness.noise_std has %d values, the observation mirror table %d" % (len(ns), len(src)))
    for c, (v, j) in enumerate(zip(ns, src)):
        if float(ns[int(j)]) != float(v):
            raise ValueError("PPO.smoothness.noise_std is not invariant under the observation mirror table: column %d has %r, its mirror "
                             "column %d has %r (PPO.mirror_loss_coef > 0 with spatial_coef > 0 needs a left-right symmetric perturbation)"
                             % (c, float(v), int(j), float(ns[int(j)])))
