"""Shared by tests/test_rnd.py (CPU), tests/test_rnd_gpu.py and tests/test_rnd_runner_gpu.py (-m gpu): a float64 restatement of
hgym_rnd_rewards, written from the text of include/hgym.h (not from the kernels), the weight schedule on the host, and the header's
size macro.  numpy only."""
import numpy as np

CONSTANT, STEP, LINEAR = 0, 1, 2          # HGYM_RND_CONSTANT / _STEP / _LINEAR
HEADER, ENVS_PER_PARTIAL, ROWS_PER_WG, APPLY_WGS = 16, 64, 64, 1024
MEAN, VAR, COUNT, COUNTER, SUM_INTRINSIC, SUM_REWARDS, WEIGHT_LAST, STD, ROWS = range(9)
MAX_OUTPUTS = 64


def block_doubles(n):
    """HGYM_RND_BLOCK_DOUBLES(n)."""
    n = int(n)
    return HEADER + n + 2 * ((n + ENVS_PER_PARTIAL - 1) // ENVS_PER_PARTIAL) + 2 * APPLY_WGS


def weight(c, schedule=CONSTANT, w0=1.0, final_value=0.0, initial_step=0, final_step=0):
    """The header's weight of step count c, in python doubles, the linear form evaluated left to right."""
    c = int(c)
    if schedule == STEP:
        return float(w0) if c < final_step else float(final_value)
    if schedule == LINEAR:
        if c <= initial_step:
            return float(w0)
        if c >= final_step:
            return float(final_value)
        return float(w0) + (float(final_value) - float(w0)) * float(c - initial_step) / float(final_step - initial_step)
    return float(w0)


def host_block(n):
    """What hgym_rnd_block_init leaves, as host doubles: mean 0, var 1, everything else 0 (for calls that must fail before any launch)."""
    b = np.zeros(block_doubles(n), dtype=np.float64)
    b[VAR] = 1.0
    return b


def fresh_state(n):
    return dict(mean=0.0, var=1.0, count=0.0, counter=0, G=np.zeros(int(n), dtype=np.float64))


def merge(mean, var, count, values):
    """The header's merge of ONE batch (population variance clamped at 0) into (mean, var, count); float64."""
    v = np.asarray(values, dtype=np.float64).ravel()
    nb = float(v.size)
    mu_b = float(v.sum()) / nb
    var_b = max(float((v * v).sum()) / nb - mu_b * mu_b, 0.0)
    count = count + nb
    rate = nb / count
    d = mu_b - mean
    mean = mean + rate * d
    var = var + rate * (var_b - var + d * (mu_b - mean))
    return mean, var, count


def scales(T, counter, std, normalize=True, **sched):
    """scale_t of every row, as the fp32 numbers the pass multiplies with."""
    out = np.empty(int(T), dtype=np.float32)
    for t in range(int(T)):
        w = weight(int(counter) + t + 1, **sched)
        out[t] = np.float32(w / std if (normalize and std > 0.0) else w)
    return out


def exact_error(pred, target):
    """The raw error of (T, n, K) embeddings in float64."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return np.sqrt(((target - pred) ** 2).sum(axis=2))


def reference(pred, target, rewards, state, gamma=0.99, normalize=True, err=None, **sched):
    """The whole pass in float64 where the header says fp64 and with the exact (float64) raw error where it says fp32.
    pred, target (T, n, K); rewards (T, n); state: fresh_state() or what an earlier call returned (not modified).
    err: (T, n) raw errors to continue from instead of the exact ones (a device's fp32 errors: everything behind them is fp64 on
    both sides, so it can be held to fp64 bars); pred and target are then not read.
    -> dict(err (float64), G_all (T, n), state (after), std, scale (T,) fp32, intrinsic (float64: err * scale), w_last)."""
    err = exact_error(pred, target) if err is None else np.asarray(err, dtype=np.float64)
    T, n = err.shape
    g = state["G"].astype(np.float64).copy()
    G_all = np.empty((T, n), dtype=np.float64)
    for t in range(T):
        g = gamma * g + err[t]
        G_all[t] = g
    mean, var, count = merge(state["mean"], state["var"], state["count"], G_all)
    std = float(np.sqrt(var))
    sc = scales(T, state["counter"], std, normalize, **sched)
    intrinsic = err * sc.astype(np.float64)[:, None]
    after = dict(mean=mean, var=var, count=count, counter=int(state["counter"]) + T, G=g)
    return dict(err=err, G_all=G_all, state=after, std=std, scale=sc, intrinsic=intrinsic,
                w_last=weight(int(state["counter"]) + T, **sched))


def err_bound(K):
    """Relative bound of the fp32 raw error against its exact value: a K-term fp32 sum of non-negative terms plus one square root
    (differences and squares included in the issue's (K + 2) units)."""
    return (int(K) + 2) * 2.0 ** -24
