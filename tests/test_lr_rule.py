"""The adaptive-KL learning-rate rule (ppo.py:140-145) at its thresholds: oracle.adapt_lr against the reference's own expression, a 0-dim
fp32 torch tensor compared with python floats.  torch rounds the python float to the tensor's dtype, so the thresholds are
float32(desired_kl * 2) and float32(desired_kl / 2) -- a python-double comparison disagrees exactly on the values between those and the
doubles (float32(0.005) = 0.004999999888 < 0.005)."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as P


def reference_rule(lr, kl_mean, desired_kl):
    """ppo.py:140-145 as written: kl_mean a 0-dim fp32 tensor, learning_rate a python float, 1e-5 / 1e-2 the clamps."""
    if kl_mean > desired_kl * 2.0:
        lr = max(1e-5, lr / 1.5)
    elif kl_mean < desired_kl / 2.0 and kl_mean > 0.0:
        lr = min(1e-2, lr * 1.5)
    return lr


def boundary_kls(desired_kl):
    """Both thresholds, their fp32 neighbours two ulps either side, the python doubles and the doubles next to them (which round to the
    fp32 thresholds), 0, -0, a negative value, NaN, +-inf and the smallest subnormal."""
    out = []
    for thr in (desired_kl * 2.0, desired_kl / 2.0):
        f = np.float32(thr)
        v = f
        for _ in range(2):
            v = np.nextafter(v, np.float32(np.inf))
            out.append(float(v))
        v = f
        for _ in range(2):
            v = np.nextafter(v, np.float32(-np.inf))
            out.append(float(v))
        out += [float(f), thr, float(np.nextafter(thr, 1.0)), float(np.nextafter(thr, 0.0))]
    return out + [0.0, -0.0, -1e-3, float("nan"), float("inf"), float("-inf"), float(np.nextafter(np.float32(0), np.float32(1)))]


DESIRED = [0.01, 0.02, 0.003, 1.0 / 3.0]


@pytest.mark.parametrize("desired_kl", DESIRED)
@pytest.mark.parametrize("lr", [1e-3, 1e-5, 1e-2, 9e-3, 1.2e-5])
def test_adapt_lr_matches_the_reference_on_the_thresholds(desired_kl, lr):
    for kl in boundary_kls(desired_kl):
        t = torch.tensor(kl, dtype=torch.float32)
        want = reference_rule(lr, t, desired_kl)
        got = P.adapt_lr(lr, t, desired_kl)
        assert got == want, "desired_kl=%r lr=%r kl=%r: oracle %r, reference %r" % (desired_kl, lr, kl, got, want)


def test_float32_half_threshold_keeps_the_rate():
    """The case the python-double comparison got wrong: float32(0.005) is not below float32(0.005)."""
    t = torch.tensor(0.005, dtype=torch.float32)
    assert reference_rule(1e-3, t, 0.01) == 1e-3
    assert P.adapt_lr(1e-3, t, 0.01) == 1e-3
    assert P.adapt_lr(1e-3, float(t), 0.01) == 1e-3


@pytest.mark.parametrize("desired_kl", DESIRED)
def test_adapt_lr_matches_the_reference_on_random_values(desired_kl):
    """10^5 fp32 KL values spread log-uniformly over [desired_kl / 8, desired_kl * 8], with a chained learning rate so that both clamps
    are reached."""
    g = torch.Generator().manual_seed(int(desired_kl * 1e6))
    kls = (desired_kl * torch.exp2((torch.rand(100000, generator=g, dtype=torch.float64) * 6 - 3))).float()
    lr_ref = lr = 1e-3
    hits = {"up": 0, "down": 0, "keep": 0, "lo": 0, "hi": 0}
    for t in kls:
        new_ref = reference_rule(lr_ref, t, desired_kl)
        lr = P.adapt_lr(lr, t, desired_kl)
        hits["up" if new_ref > lr_ref else "down" if new_ref < lr_ref else "keep"] += 1
        lr_ref = new_ref
        hits["lo"] += lr_ref == 1e-5
        hits["hi"] += lr_ref == 1e-2
        assert lr == lr_ref
    assert min(hits.values()) > 0, hits
