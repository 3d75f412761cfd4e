"""PPO.exploration_noise: temporally correlated action noise.

The reference samples a_t = mu_t + sigma z_t with z_t white: fresh normals at every vec-step.  At a 100 Hz control rate that is joint jitter
which averages out within a gait phase.  With the option on the normals of one rollout are a filtered sequence per (env, action),

    x_t = carry[t] * state + sum_{s <= t} filt[t][s] * w_s,        a_t = mu_t + sigma x_t,

w_s being exactly the white draws the policy launches would have made (same Philox key, counter and Box-Muller pairing).  filt is lower
triangular with rows of unit norm (carry included), so every x_t is marginally N(0, 1): the log-probability, the stored sigma, the ratio and the
update keep their formulas -- PPO goes on treating the steps as independent, as "Colored Noise in PPO" (Hollenstein et al., AAAI 2024) does;
that is the option's one deviation.  Two filters, built here in float64 and rounded to fp32 once:

    {"kind": "ar1", "rho": r}, 0 <= r < 1         filt[t][s] = sqrt(1 - r^2) r^(t-s), carry[t] = r^(t+1): a stationary Ornstein-Uhlenbeck
                                                  sequence that continues across rollouts through `state` ((n, A), x of the last step)
    {"kind": "colored", "beta": b}, 0 <= b <= 2   filt = cholesky(Toeplitz(r)), r(k) = sum_i f_i^-b cos(2 pi f_i k) / sum_i f_i^-b over the
                                                  midpoint frequencies f_i = (i - 1/2) / (2 M), i = 1 .. M = 4 T: power ~ f^-b, every
                                                  rollout a fresh sequence (no carry)

rho = 0 and beta = 0 give the exact identity and no carry: the plumbing with the reference's noise.  The same filter serves every env and
action.  The sequence does not restart where an episode ends: the table is made before the rollout knows its resets; the marginal is
unaffected.  One launch (hgym_policy_noise_table) fills the table at the head of every rollout, inside the captured rollout graph; each policy
launch then reads its row in place of its own draw (`z` of hgym_policy_act / _fin, hgym_rollout_step_z).  Nothing in the update sees the option.
"""
import ctypes as C
import math

import torch

MAX_STEPS = 128      # HGYM_NOISE_MAX_STEPS
MAX_ACTIONS = 12     # HGYM_NUM_ACTIONS
SIDECAR_KEY = "exploration_noise"      # what the exact-resume sidecar of a run with an AR(1) filter carries beside the env's state
KINDS = {"ar1": ("rho", 0.0, 1.0, False), "colored": ("beta", 0.0, 2.0, True)}      # kind -> (its parameter, lo, hi, hi included?)


# ------------------------------------------------------------------ configuration
def parse_config(cfg):
    """PPO.exploration_noise -> {"kind", "param" (the parameter's name), "value"}, or None (off: None).  ValueError: not a dict, no or an
    unknown kind, an unknown key (named), the kind's parameter missing, not finite or outside its range."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("PPO.exploration_noise=%r: a dict {\"kind\": \"ar1\", \"rho\": r} or {\"kind\": \"colored\", \"beta\": b}, or None" % (cfg,))
    kind = cfg.get("kind")
    if kind not in KINDS:
        raise ValueError("PPO.exploration_noise: kind=%r is not one of %s" % (kind, ", ".join(sorted(KINDS))))
    name, lo, hi, closed = KINDS[kind]
    unknown = sorted(set(cfg) - {"kind", name})
    if unknown:
        raise ValueError("PPO.exploration_noise: unknown key %r for kind %r (its keys: kind, %s)" % (unknown[0], kind, name))
    if name not in cfg:
        raise ValueError("PPO.exploration_noise: kind %r needs %r" % (kind, name))
    try:
        v = float(cfg[name])
    except (TypeError, ValueError):
        raise ValueError("PPO.exploration_noise: %s=%r is not a number" % (name, cfg[name]))
    if not (math.isfinite(v) and lo <= v and (v <= hi if closed else v < hi)):
        raise ValueError("PPO.exploration_noise: %s=%r outside [%g, %g%s" % (name, cfg[name], lo, hi, "]" if closed else ")"))
    return dict(kind=kind, param=name, value=v)


def config_from_env(environ):
    """HGYM_NOISE_COLOR=<beta> / HGYM_NOISE_AR1=<rho> -> `algorithm.exploration_noise_cfg`, or None when neither is set.  Both: ValueError."""
    color, ar1 = environ.get("HGYM_NOISE_COLOR"), environ.get("HGYM_NOISE_AR1")
    if color and ar1:
        raise ValueError("HGYM_NOISE_COLOR=%r and HGYM_NOISE_AR1=%r: one filter at a time" % (color, ar1))
    if color:
        return {"kind": "colored", "beta": float(color)}
    if ar1:
        return {"kind": "ar1", "rho": float(ar1)}
    return None


def check_setup(num_transitions_per_env, num_actions):
    """What init_storage refuses with the option on (ValueError): a rollout longer than the table launch fills, more actions than it knows."""
    if int(num_transitions_per_env) > MAX_STEPS:
        raise ValueError("PPO.exploration_noise: num_steps_per_env=%d exceeds the %d steps one noise table holds" % (num_transitions_per_env, MAX_STEPS))
    if not 1 <= int(num_actions) <= MAX_ACTIONS:
        raise ValueError("PPO.exploration_noise: num_actions=%d outside [1, %d]" % (num_actions, MAX_ACTIONS))


# ------------------------------------------------------------------ the filters, float64
def ar1_filter(T, rho):
    """(filt (T, T), carry (T,)) in float64: filt[t][s] = sqrt(1 - rho^2) rho^(t-s) for s <= t, carry[t] = rho^(t+1), so that
    filt filt^T + carry carry^T = rho^|t-s|.  rho == 0: (the exact identity, None)."""
    T, rho = int(T), float(rho)
    if rho == 0.0:
        return torch.eye(T, dtype=torch.float64), None
    pw = torch.tensor([rho ** k for k in range(T + 1)], dtype=torch.float64)      # (python's pow, entry by entry: the same bits at every T)
    t = torch.arange(T)
    lag = t[:, None] - t[None, :]
    filt = torch.where(lag >= 0, math.sqrt(1.0 - rho * rho) * pw[lag.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    return filt, pw[1:].clone()


def colored_autocorrelation(T, beta, lags=None):
    """r(k), k = 0 .. lags - 1 (default T), float64: sum_i f_i^-beta cos(2 pi f_i k) / sum_i f_i^-beta, f_i = (i - 1/2) / (2 M), M = 4 T."""
    T, beta = int(T), float(beta)
    M = 4 * T
    f = (torch.arange(1, M + 1, dtype=torch.float64) - 0.5) / (2.0 * M)
    p = torch.pow(f, -beta)
    k = torch.arange(T if lags is None else int(lags), dtype=torch.float64)
    return (torch.cos(2.0 * math.pi * k[:, None] * f[None, :]) * p[None, :]).sum(dim=1) / p.sum()


def colored_filter(T, beta):
    """(filt (T, T), None) in float64: the Cholesky factor of Toeplitz(colored_autocorrelation(T, beta)).  beta == 0: the exact identity."""
    T, beta = int(T), float(beta)
    if beta == 0.0:
        return torch.eye(T, dtype=torch.float64), None
    r = colored_autocorrelation(T, beta)
    t = torch.arange(T)
    return torch.linalg.cholesky(r[(t[:, None] - t[None, :]).abs()]), None


def build_filter(cfg, T):
    """parse_config's dict -> (filt, carry or None) in float64 for rollouts of up to T steps; a shorter rollout uses the leading block."""
    return ar1_filter(T, cfg["value"]) if cfg["kind"] == "ar1" else colored_filter(T, cfg["value"])


def lag1(cfg, T):
    """The configured correlation of x_t and x_{t+1}: rho, or the coloured filter's r(1) at storage length T."""
    if cfg["value"] == 0.0:
        return 0.0
    return cfg["value"] if cfg["kind"] == "ar1" else float(colored_autocorrelation(T, cfg["value"], lags=2)[1])


# ------------------------------------------------------------------ the reference twin
def table_reference(filt, carry, state, w, dtype=torch.float32):
    """What hgym_policy_noise_table computes, in torch on `w`'s device: w (T, ...) the raw draws, state (...) or None, filt (T, T) and carry
    (T,) or None (any float dtype: cast to `dtype` first).  dtype float32: the kernel's bits -- x = carry * state (+0 without a carry), then
    x = x + filt[t][s] * w_s for s ascending, one rounding per multiply and per add.  float64: the same sums in double precision.  Returns
    (x (T, ...), bound (T, ...)): bound = sum |coefficient * term| in `dtype`, for the fp32-against-float64 bound (t + 2) 2^-24 bound[t]."""
    T = w.shape[0]
    tail = (1,) * (w.dim() - 1)
    w = w.to(dtype)
    f = filt.to(dtype).to(w.device)
    x, bound = torch.zeros_like(w), torch.zeros_like(w)
    if carry is not None:
        c = carry.to(dtype).to(w.device).view(T, *tail)
        x = (c * state.to(dtype)).contiguous()
        bound = x.abs()
    for s in range(T):      # term s joins every row t >= s: per row the terms arrive in ascending s
        term = f[s:, s].view(T - s, *tail) * w[s]
        x[s:] = x[s:] + term
        bound[s:] = bound[s:] + term.abs()
    return x, bound


# ------------------------------------------------------------------ the option
class ExplorationNoise:
    """The option as PPO holds it (PPO._noise; None: off): the fp32 filter and carry on the device, the AR(1) state, the table of one rollout,
    the launch, the rollout graph key's entry and the state a sidecar carries."""

    def __init__(self, cfg, num_transitions_per_env, num_envs, num_actions, device, seed=0):
        from hgym import _lib as L
        self._L = L
        check_setup(num_transitions_per_env, num_actions)
        self.cfg, self.T, self.n, self.A, self.device = dict(cfg), int(num_transitions_per_env), int(num_envs), int(num_actions), device
        filt, carry = build_filter(cfg, self.T)
        self.filt = filt.to(torch.float32).contiguous().to(device)           # rounded to fp32 once
        self.carry = None if carry is None else carry.to(torch.float32).contiguous().to(device)
        self.state = None
        if self.carry is not None:      # a stationary start: x_{-1} ~ N(0, 1), from the run's seed
            g = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
            self.state = torch.randn(self.n, self.A, generator=g, dtype=torch.float32).to(device)
        self.table = torch.zeros(self.T, self.n, self.A, dtype=torch.float32, device=device)
        self.lag1 = lag1(cfg, self.T)
        self._logged = False

    def fill(self, step, seed, T=None):
        """The table of a rollout of T steps (default: the storage's) whose first policy launch samples at step `step[0]` (a device int64,
        read by the launch): rows 0 .. T - 1 of `table`; the state moves on to x_{T-1}.  One launch on the current stream, capturable."""
        L = self._L
        T = self.T if T is None else int(T)
        L.check(L.lib.hgym_policy_noise_table(T, self.n, self.A, L.fptr(self.filt), self.T, L.fptr(self.carry), L.fptr(self.state),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, L.i64ptr(step), L.fptr(self.table),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_policy_noise_table")

    def row(self, t):
        return self.table[t]

    def graph_key(self):
        return ("exploration_noise", self.cfg["kind"], self.cfg["value"], self.table.data_ptr())

    def log_scalars(self):
        """Policy/noise_lag1, the configured lag-1 correlation: once."""
        if self._logged:
            return []
        self._logged = True
        return [("Policy/noise_lag1", float(self.lag1))]

    # ------------------------------------------------------------------ the exact-resume sidecar
    def state_dict(self, out=None):
        """{kind, value, state} with the AR(1) state on the host, or None when the filter carries nothing across rollouts.  out: a pinned
        host tensor of the state's shape (the background checkpoint path keeps one per snapshot buffer set) -- the copy is then
        stream-ordered and complete behind the caller's next event."""
        if self.state is None:
            return None
        if out is not None:
            host = out
            host.copy_(self.state, non_blocking=True)
        else:
            host = self.state.cpu()
        return dict(kind=self.cfg["kind"], value=self.cfg["value"], state=host)

    def check_state_dict(self, sd):
        """A sidecar's entry that does not fit this run's table: ValueError before anything is changed.  None (a run without a carried state) fits."""
        if sd is None or self.state is None:
            return
        if tuple(sd["state"].shape) != tuple(self.state.shape):
            raise ValueError("exploration noise state: shape %s in the sidecar, %s here" % (tuple(sd["state"].shape), tuple(self.state.shape)))

    def load_state_dict(self, sd):
        if sd is None or self.state is None:
            return
        with torch.inference_mode():
            self.state.copy_(sd["state"].to(torch.float32))
