"""The smoothness regulariser on the policy's mean (PPO.smoothness): the configuration and what init_storage refuses,
as functions that need no device.

PPO.smoothness = None | dict with the keys of DEFAULTS:
  temporal_coef  lamT >= 0: pulls mu(s_t) towards mu(s_t+1) (rows whose episode ended weigh 0)
  spatial_coef   lamS >= 0: pulls mu(s) towards mu(s + noise_std * z)
  noise_std      a scalar or a (num_obs,) vector, raw observation units; needed with spatial_coef > 0 (OnPolicyRunner fills it with the env's
                 noise_scale_vec * noise_level tiled over the stacked frames)
  noise_scale    a factor on noise_std (default 1.0)
  seed           the Philox key of the perturbation (default: the run's seed)
None, or both coefficients 0: off."""
import math

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
    rank; PPO.symmetry in any form (the mirrored half stores no mirrored bootstrap slot, and the mirror head and this head are separate
    kernels); Distillation."""
    if int(world) > 1:
        raise ValueError("PPO.smoothness runs on one rank (world size %d)" % int(world))
    if symmetry is not None:
        raise ValueError("PPO.smoothness does not support PPO.symmetry (augmentation or mirror loss)")
    if distillation:
        raise ValueError("PPO.smoothness does not support Distillation")


def graph_key(cfg, buffers):
    """PPO.update_graph_key's entry: the coefficients and the seed of a parse_config() dict (None: off) and the scratch the launches name
    (RolloutStorage.smooth_buffers)."""
    if cfg is None:
        return None
    return (cfg["temporal_coef"], cfg["spatial_coef"], cfg["seed"]) + tuple(t.data_ptr() for t in buffers)


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
