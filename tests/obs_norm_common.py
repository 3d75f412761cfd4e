"""Shared by tests/test_obs_norm.py (CPU) and tests/test_obs_norm_gpu.py / tests/test_obs_norm_runner_gpu.py (-m gpu): float64 numpy
restatements of the observation normaliser (csrc/hgym_norm.hip) -- the merge of a batch into the running statistics,
the floats the kernels read, the fold of the statistics into a first layer and the unfold of its gradient -- and the error bounds the GPU
tests hold the device against.

Bounds (u = 2^-53, the fp64 unit roundoff; M = rows of the batch; both per merge).  The device forms sum x and sum x^2 in fp64 in some fixed
order; any order of M additions of numbers bounded by X has an error below (M - 1) u M X (Higham, Accuracy and Stability, (4.4)), so
  mu_b = sum x / M          is within  M u max|x|                       of the exact mean, plus one rounding of the division;
  sum x^2 / M               is within  M u max x^2                      of the exact mean square;
  mu_b^2                    moves by   2 |mu_b| M u max|x| <= 2 M u max x^2;
the reference's own two-pass variance carries the same kind of error (<= (M + 2) u max x^2).  The merge multiplies both by rate <= 1 and adds
a handful of roundings of quantities bounded by max x^2.  |d mean| <= 4 M u max|x| and |d var| <= 16 M u max x^2 cover that with room, for
M = 1 as well (there both sides compute x^2 - x^2 = 0 exactly)."""
import numpy as np

U = 2.0 ** -53


def initial(K):
    """rsl_rl's EmpiricalNormalization at construction: mean 0, var 1, count 0."""
    return dict(mean=np.zeros(K), var=np.ones(K), count=0.0)


def merge(state, x, until=None):
    """One batch x (M, K) into state (mean, var, count): rsl_rl's update with the batch's population statistics taken in float64 (two
    passes).  until: once count >= until the batch is skipped.  Returns a new state."""
    x = np.asarray(x, np.float64)
    if until is not None and state["count"] >= until:
        return dict(mean=state["mean"].copy(), var=state["var"].copy(), count=state["count"])
    n = float(x.shape[0])
    mu_b = x.mean(axis=0)
    var_b = np.maximum(((x - mu_b) ** 2).mean(axis=0), 0.0)
    count = state["count"] + n
    rate = n / count
    d = mu_b - state["mean"]
    mean = state["mean"] + rate * d
    var = state["var"] + rate * (var_b - state["var"] + d * (mu_b - mean))
    return dict(mean=mean, var=var, count=count)


def bounds(x):
    """(bound on |d mean|, bound on |d var|) of one merge of batch x, per the module docstring."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    return 4.0 * M * U * np.abs(x).max(), 16.0 * M * U * (x ** 2).max()


def derived(mean, var, eps):
    """The kernels' floats: m = (float)mean, s = (float)(1 / (sqrt(var) + (double)(float)eps))."""
    e = float(np.float32(eps))
    return np.asarray(mean, np.float64).astype(np.float32), (1.0 / (np.sqrt(np.asarray(var, np.float64)) + e)).astype(np.float32)


def bf16(a):
    """fp32 -> bf16 (round to nearest even) -> fp32, numpy."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def operand(W, s, precision):
    """Wop = T(w * s[c]): the fp32 product, rounded to the operand type (fp32 arrays in, fp32 array out)."""
    ws = np.asarray(W, np.float32) * np.asarray(s, np.float32)[None, :]
    return bf16(ws) if precision == "bf16" else ws


def fold(W, b, m, s, precision):
    """(Wop, b') of a first layer (W (N, K), b (N,)) under statistics m, s (K,): b' = b - Wop m in float64 (not yet rounded to fp32).
    |W|m: sum_c |Wop[r, c] m[c]|, the scale of the bound 2^-23 (|b| + sum |Wop m|) on the device's fp32 effective bias."""
    Wop = operand(W, s, precision)
    prod = Wop.astype(np.float64) * np.asarray(m, np.float64)[None, :]
    return Wop, np.asarray(b, np.float64) - prod.sum(axis=1), np.abs(prod).sum(axis=1)


def unfold(GW, gb, m, s):
    """G_W[r, c] = (G'_W[r, c] - g_b[r] m[c]) s[c] in float64."""
    GW, gb, m, s = (np.asarray(a, np.float64) for a in (GW, gb, m, s))
    return (GW - gb[:, None] * m[None, :]) * s[None, :]


def normalise(x, m, s):
    """(x - m) s in float64 from the kernels' floats: the rows a net WITHOUT the fold would have to be fed."""
    return (np.asarray(x, np.float64) - np.asarray(m, np.float64)[None, :]) * np.asarray(s, np.float64)[None, :]
