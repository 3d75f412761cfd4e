"""Shared by tests/test_value_norm.py (CPU), tests/test_value_norm_gpu.py and tests/test_value_norm_runner_gpu.py (-m gpu): value-target
normalisation (PPO.value_normalization) restated in numpy from the text of include/hgym.h -- nothing here calls the
library.

  batch_stats   n, mean and population variance of a batch in float64, two passes (the mean, then the squared deviations from it)
  merge         rsl_rl's EmpiricalNormalization merge in float64, as the header states it (from count = 0: the batch's statistics themselves)
  floats        mean_f = (float)mean, scale_f = (float)sqrt(var) + eps
  denormalize   V = v * scale_f + mean_f        fp32, two roundings (numpy rounds every fp32 operation once: IEEE, no fma)
  normalize     y = (x - mean_f) / scale_f      fp32, two roundings"""
import math

import numpy as np

INITIAL = (0.0, 0.0, 1.0)      # count, mean, var
EPS = 1e-2                     # PPO.value_normalization_eps' default
CHUNK, MAX_BLOCKS = 1024, 1024      # HGYM_VALUE_NORM_CHUNK, HGYM_VALUE_NORM_MAX_BLOCKS
U = 2.0 ** -53                 # float64's unit roundoff


def scratch_doubles(n):
    """HGYM_VALUE_NORM_SCRATCH_DOUBLES(n)."""
    return 4 + 2 * ((int(n) + CHUNK - 1) // CHUNK)


def batch_stats(x):
    """(n, mean, var) of the values x in float64: math.fsum for both passes (exactly rounded sums), population variance."""
    a = np.asarray(x, dtype=np.float64).reshape(-1)
    n = float(a.size)
    mean = math.fsum(a.tolist()) / n
    var = math.fsum(((a - mean) ** 2).tolist()) / n
    return n, mean, var


def merge(state, batch):
    """state = (count, mean, var), batch = (n, mean_b, var_b) -> the merged state, float64 python arithmetic."""
    count, mean, var = state
    n, mean_b, var_b = batch
    count_new = count + n
    if not count > 0.0:
        return count_new, mean_b, var_b
    rate = n / count_new
    d = mean_b - mean
    mean_new = mean + rate * d
    var_new = var + rate * (var_b - var + d * (mean_b - mean_new))
    return count_new, mean_new, max(var_new, 0.0)


def floats(state, eps=EPS):
    """(mean_f, scale_f) as numpy float32 scalars."""
    _, mean, var = state
    return np.float32(mean), np.float32(np.float32(math.sqrt(var)) + np.float32(eps))


def denormalize(v, state, eps=EPS):
    mean_f, scale_f = floats(state, eps)
    out = np.asarray(v, dtype=np.float32) * scale_f
    return out + mean_f


def normalize(x, state, eps=EPS):
    mean_f, scale_f = floats(state, eps)
    out = np.asarray(x, dtype=np.float32) - mean_f
    return out / scale_f


def rel(got, want):
    """|got - want| relative to |want| (absolute where want is 0)."""
    return abs(got - want) / (abs(want) if want != 0.0 else 1.0)
