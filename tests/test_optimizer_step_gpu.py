"""-m gpu: the optimiser side of the update at its edges -- the squared gradient norm reduce_slabs_kernel leaves in opt[9], clip_grad_norm_
+ Adam (ppo.py:173-174) over hundreds and thousands of steps, and the adaptive-KL learning rate (ppo.py:140-145) on its thresholds, in
hgym_ppo_apply's prologue and in the fused gradient call's (grad_norm_ready).

References, all float64 and restated here:
  * the learning-rate rule as the reference evaluates it: kl_mean a 0-dim fp32 tensor compared with python floats (torch rounds them to
    fp32), the rate a python double clamped to [1e-5, 1e-2];
  * one Adam step (torch.optim.Adam defaults) after clip_grad_norm_, taken from the kernel's own previous parameters and moments (read
    back before the step, so that error does not compound) with the hyperparameters the C-ABI carries (fp32 beta1, beta2, eps: 1 - beta2
    is formed from the fp32 beta2, as adam_kernel forms it).
Element-wise bounds, u = 2^-24: |m - m64| <= 8u (|beta1 m_old| + |(1 - beta1) g|) (g carries the fp32 clip coefficient, <= 5u);
|v - v64| <= 16u v64 (each plus 8 x 2^-149 for subnormal results); |p - p64| <= half an fp32 ulp of p + 16u |step64| + step_size |m - m64|-bound / denom64."""
import math

import numpy as np
import pytest
import torch

import bf16_report as BR
import layer_path_common as LP
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SUB = 8 * 2.0 ** -149       # below 2^-126 an fp32 rounding errs by up to 2^-150 absolute, not u relative (v of a ~1e-17 gradient element)
LR_MIN, LR_MAX = 1e-5, 1e-2
XBOTL = (705, 219, 12, [512, 256, 128], [768, 256, 128])


def reference_lr(lr, kl, desired_kl):
    """ppo.py:140-145 as written, kl_mean the fp32 tensor the reference has."""
    kl_mean = torch.tensor(float(np.float32(kl)), dtype=torch.float32)
    if kl_mean > desired_kl * 2.0:
        lr = max(LR_MIN, lr / 1.5)
    elif kl_mean < desired_kl / 2.0 and kl_mean > 0.0:
        lr = min(LR_MAX, lr * 1.5)
    return lr


def f32_ulps(a, b):
    """distance of two floats in fp32 ulps of b"""
    return abs(a - b) / float(np.spacing(np.float32(abs(b))))


def _net(kind, max_batch, seed, lr):
    from hgym import NetBuffers, make_net_config
    g = torch.Generator().manual_seed(seed)
    if kind == "fused":
        no, npv, A, ah, ch = XBOTL
        cfg = make_net_config(no, npv, A, ah, ch, "bf16", max_batch)
    else:
        name, precision = kind.split("-")
        no, npv, A, ah, ch = LP.CASES[name][:5]
        cfg = LP.net_config(name, precision, max_batch)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    net = NetBuffers(cfg, "cuda", learning_rate=lr)
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    if kind == "fused":
        assert net.shadow_ld(0) > 0                 # the fused bf16 layout
    else:
        assert net.shadow_ld(0) == 0
    torch.cuda.synchronize()
    return p, net, g, (no, npv, A)


def _batch_cols(p, dims, S, g, ret_shift=0.0, zero_adv=False):
    no, npv, A = dims
    obs, priv = torch.randn(S, no, generator=g), torch.randn(S, npv, generator=g)
    act, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g) + ret_shift
    if zero_adv:
        adv.zero_()
    with torch.no_grad():
        mu_now = P.mlp_forward(obs, p.actor)
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    return [t.cuda().contiguous() for t in (obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o)]


def _adam64(p_old, m_old, v_old, G, sq64, t, lr, max_norm, beta1, beta2, eps):
    """clip_grad_norm_ + one torch.optim.Adam step in float64 from the given state; returns (p, m, v, bounds p, m, v, coef)."""
    b1, b2, eps = float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(eps))
    total = math.sqrt(sq64)
    coef = min(float(np.float32(max_norm)) / (total + 1e-6), 1.0)
    g = G * coef
    m = b1 * m_old + (1.0 - b1) * g
    v = b2 * v_old + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    ss = lr / bc1
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    step = -ss * m / denom
    p = p_old + step
    bm = 8 * U * (np.abs(b1 * m_old) + np.abs((1.0 - b1) * g)) + SUB
    bv = 16 * U * v + SUB
    bp = 0.5 * np.spacing(np.maximum(np.abs(p), np.abs(p_old)).astype(np.float32)).astype(np.float64) + 16 * U * np.abs(step) \
        + ss * bm / denom
    return p, m, v, bp, bm, bv, coef


def _state(net):
    return [t.double().cpu().numpy() for t in (net.params, net.adam_m, net.adam_v)]


def _check_step(before, after, G, sq64, t, lr, ppo, what):
    """after == one float64 clip + Adam step from `before`, element-wise within the derived bounds; returns the worst err / bound."""
    p64, m64, v64, bp, bm, bv, coef = _adam64(*before, G, sq64, t, lr, ppo.max_grad_norm, ppo.beta1, ppo.beta2, ppo.adam_eps)
    worst = 0.0
    for name, got, ref, b in (("params", after[0], p64, bp), ("adam_m", after[1], m64, bm), ("adam_v", after[2], v64, bv)):
        r = float((np.abs(got - ref) / b).max())
        assert r <= 1.0, "%s: %s worst |kernel - float64| / bound = %.3g" % (what, name, r)
        worst = max(worst, r)
    return worst, coef


def _nwg(net):
    return 96 * len(net.views)          # reduce_slabs_kernel: RSN_X = 96 workgroups per parameter segment


# ---------------------------------------------------------------------------------------------- 1. gradient norm regimes
REGIMES = {
    # name: (returns shift, zero advantages, value_loss_coef, entropy_coef, max_grad_norm as a multiple of the measured norm)
    "unit_clipped": (0.0, False, 1.0, 0.001, 0.5),
    "unit_unclipped": (0.0, False, 1.0, 0.001, 2.0),
    "large": (1e3, False, 1.0, 0.001, None),          # value-loss gradient ~1e3: squared norm >> 128, fp64 sums round in arrival order
    "tiny": (0.0, True, 1e-9, 0.0, None),             # squared norm ~1e-18: every workgroup's partial below the 2^-46 quantum
}


@pytest.mark.parametrize("kind", ["fused", "deep-f32"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_grad_norm_and_step_in_every_regime(kind, regime):
    """hgym_ppo_grad (grad_norm_ready: the norm comes from reduce_slabs_kernel's pre-rounded fp64 atomics) then hgym_ppo_apply.
    opt[9] against the float64 squared norm of the kernel's own gradient: |err| <= nwg 2^-47 (the quantum rounding, the kernel's stated
    bound) + (nwg + 128) 2^-53 sq (fp64 additions in the workgroup and, above 128, the arrival-order atomics); opt[6] = fp32 sqrt(opt[9]);
    the step = float64 clip_grad_norm_ + Adam on that gradient."""
    from hgym import make_ppo_config, make_batch
    shift, zero_adv, vcoef, ecoef, mult = REGIMES[regime]
    S, B = 5000, 4096
    p, net, g, dims = _net(kind, B, 31, 1e-3)
    cols = _batch_cols(p, dims, S, g, ret_shift=shift, zero_adv=zero_adv)
    idx = torch.randperm(S, generator=g)[:B].contiguous().cuda()
    batch = make_batch(*cols, idx)
    probe = make_ppo_config(value_loss_coef=vcoef, entropy_coef=ecoef, adaptive=False)
    net.ppo_grad(probe, batch)                        # learn the norm (no prologue: grad_norm_ready off)
    torch.cuda.synchronize()
    n0 = float(net.grads.double().norm())
    max_norm = n0 * mult if mult else 1.0
    ppo = make_ppo_config(value_loss_coef=vcoef, entropy_coef=ecoef, max_grad_norm=max_norm, adaptive=False, grad_norm_ready=True)
    before = _state(net)
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    G = net.grads.double().cpu().numpy()
    sq64 = math.fsum(G * G)
    opt9 = float(net.opt_state[L.OPT_GRAD_SQNORM])
    nwg = _nwg(net)
    bound9 = nwg * 2.0 ** -47 + (nwg + 128) * 2.0 ** -53 * sq64
    what = "%s %s (|g| = %.3g)" % (kind, regime, math.sqrt(sq64))
    BR.check("opt[OPT_GRAD_SQNORM] %s: |opt[OPT_GRAD_SQNORM] - float64 sum| / derived bound" % what, abs(opt9 - sq64) / bound9, 1.0)
    if regime == "large":
        assert sq64 > 1e4
    elif regime == "tiny":
        assert sq64 < 1e-12 and abs(opt9 - sq64) <= nwg * 2.0 ** -47
    net.ppo_apply(ppo)
    torch.cuda.synchronize()
    assert float(net.opt_state[L.OPT_GRAD_NORM]) == float(np.float32(math.sqrt(opt9)))
    assert f32_ulps(float(net.opt_state[L.OPT_GRAD_NORM]), math.sqrt(sq64)) <= 1.0 or sq64 < 1e-12
    worst, coef = _check_step(before, _state(net), G, sq64, 1, 1e-3, ppo, what)
    BR.check("clip + Adam %s: worst err / derived bound" % what, worst, 1.0)
    if regime == "unit_clipped" or regime == "large":
        assert coef < 0.99
    else:
        assert coef == 1.0                            # tiny: the unclipped step (total ~ 0, coef = max_norm / 1e-6 clamped)
    assert math.isclose(float(net.opt_state[L.OPT_STEP_SIZE]), 1e-3 / (1 - float(np.float32(0.9))), rel_tol=U)


# ---------------------------------------------------------------------------------------------- 2. a long trajectory of hgym_ppo_apply
def _kl_schedule(desired_kl, n, g):
    """Threshold values (fp32 thresholds, their fp32 neighbours, float64 values that round onto them), 0, a negative value, NaN, and
    plain raise / keep / lower values; the first half leans to raising (lr_max is reached and held), the second to lowering (lr_min)."""
    hi, lo = np.float32(desired_kl) * np.float32(2), np.float32(desired_kl) * np.float32(0.5)
    edge = []
    for f in (hi, lo):
        edge += [float(f), float(np.nextafter(f, np.float32(1))), float(np.nextafter(f, np.float32(0))),
                 float(f) + float(np.spacing(f)) / 4, float(f) - float(np.spacing(f)) / 4]
    edge += [0.0, -1e-3, float("nan")]
    raise_, lower = float(lo) * 0.2, float(hi) * 3
    out = []
    for k in range(n):
        r = float(torch.rand(1, generator=g))
        if r < 0.35:
            out.append(edge[int(torch.randint(len(edge), (1,), generator=g))])
        elif k < n // 2:
            out.append(raise_ if r < 0.85 else lower)
        else:
            out.append(lower if r < 0.85 else raise_)
    return out


def _norm_schedule(n, max_norm):
    """gradient norms sweeping 1/8 .. 8 x max_grad_norm"""
    return [max_norm * 2.0 ** (3.0 * math.sin(0.37 * k)) for k in range(n)]


@pytest.mark.parametrize("kind,world", [("pad-f32", 1), ("pad-bf16", 1), ("pad-f32", 2), ("fused", 1), ("fused", 2)])
def test_apply_trajectory(kind, world):
    """320 hgym_ppo_apply steps on injected gradients (norms across max_grad_norm) and planted KL values -- through opt_state[8] with
    one rank and grad_norm_ready off, through the KL slot grads_ext[P] with world_size = 2 (gradient and KL hold the rank sum).
    Every step: opt[0] == the reference rule replayed in python, bit for bit; opt[1] == t; opt[11], opt[12] within one fp32 ulp of
    lr / (1 - beta1^t), sqrt(1 - beta2^t).  Sampled steps: params, adam_m, adam_v against the float64 step from the kernel's own state."""
    from hgym import make_ppo_config
    n = 320
    lr = 8e-3                                          # near lr_max
    p, net, g, _ = _net(kind, 512, 41 + world, lr)
    desired = 0.01
    ppo = make_ppo_config(desired_kl=desired, world_size=world)
    kls = _kl_schedule(desired, n, g)
    norms = _norm_schedule(n, ppo.max_grad_norm)
    gd = torch.Generator(device="cuda").manual_seed(43)
    pool = [torch.randn(net.P, device="cuda", generator=gd) for _ in range(3)]
    pool = [v / v.double().norm().float() for v in pool]
    seen = {"hi": 0, "lo": 0}
    worst = 0.0
    for k in range(n):
        t = k + 1
        G = pool[k % 3] * norms[k]
        if world == 1:
            net.grads.copy_(G)
            net.opt_state[L.OPT_KL_LAST] = kls[k]
        else:
            net.grads.copy_(G * world)                               # x2, x0.5: exact
            net.grads_ext[net.P] = float(np.float32(kls[k])) * world
        sampled = k < 3 or k % 29 == 0 or k == n - 1
        if sampled:
            torch.cuda.synchronize()
            before = _state(net)
            G64 = G.double().cpu().numpy()
        net.ppo_apply(ppo)
        lr = reference_lr(lr, kls[k], desired)
        seen["hi"] += lr == LR_MAX
        seen["lo"] += lr == LR_MIN
        opt = net.opt_state.cpu()
        what = "%s world=%d step %d kl=%r" % (kind, world, t, kls[k])
        assert float(opt[L.OPT_LR]) == lr, "%s: lr %r, reference %r" % (what, float(opt[L.OPT_LR]), lr)
        assert float(opt[L.OPT_STEP]) == t
        b1, b2 = float(np.float32(ppo.beta1)), float(np.float32(ppo.beta2))
        assert f32_ulps(float(opt[L.OPT_STEP_SIZE]), lr / (1 - b1 ** t)) <= 1.0, what
        assert f32_ulps(float(opt[L.OPT_SQRT_BC2]), math.sqrt(1 - b2 ** t)) <= 1.0, what
        if sampled:
            sq64 = math.fsum(G64 * G64)
            r, _ = _check_step(before, _state(net), G64, sq64, t, lr, ppo, what)
            worst = max(worst, r)
    assert seen["hi"] >= 5 and seen["lo"] >= 5, seen     # both clamps engaged and held
    BR.check("apply trajectory %s world=%d, %d steps: worst err / derived bound" % (kind, world, n), worst, 1.0)


def test_apply_5000_steps_bias_corrections():
    """5 000 cheap steps on the thinnest net (adaptive rate off): at t = 5 000, 1 - beta2^t = 0.993 and 1 - beta1^t = 1 to fp32; the
    scalars and the step stay on the float64 reference."""
    from hgym import make_ppo_config
    n = 5000
    lr = 1e-3
    p, net, g, _ = _net("thin-f32", 64, 51, lr)
    ppo = make_ppo_config(adaptive=False)
    gd = torch.Generator(device="cuda").manual_seed(53)
    pool = [torch.randn(net.P, device="cuda", generator=gd) for _ in range(4)]
    norms = _norm_schedule(n, ppo.max_grad_norm)
    samples = {1, 2, 10, 100, 1000, 2500, 4000, 4999, 5000}
    worst = 0.0
    for t in range(1, n + 1):
        G = pool[t % 4] * norms[t - 1]
        net.grads.copy_(G)
        if t in samples:
            torch.cuda.synchronize()
            before = _state(net)
            G64 = G.double().cpu().numpy()
        net.ppo_apply(ppo)
        if t in samples:
            opt = net.opt_state.cpu()
            assert float(opt[L.OPT_STEP]) == t and float(opt[L.OPT_LR]) == lr
            b1, b2 = float(np.float32(ppo.beta1)), float(np.float32(ppo.beta2))
            assert f32_ulps(float(opt[L.OPT_STEP_SIZE]), lr / (1 - b1 ** t)) <= 1.0, t
            assert f32_ulps(float(opt[L.OPT_SQRT_BC2]), math.sqrt(1 - b2 ** t)) <= 1.0, t
            r, _ = _check_step(before, _state(net), G64, math.fsum(G64 * G64), t, lr, ppo, "thin t=%d" % t)
            worst = max(worst, r)
    BR.check("apply 5000 steps thin-f32: worst err / derived bound", worst, 1.0)


# ---------------------------------------------------------------------------------------------- 3. the rule in both prologues
@pytest.mark.parametrize("side", ["upper", "lower"])
def test_boundary_kl_in_the_gradient_and_the_apply_prologue(side):
    """The minibatch KL the fused gradient call forms, put exactly on a threshold: desired_kl = kl32 / 2 (upper: 2 desired_kl = kl32) or
    2 kl32 (lower: desired_kl / 2 = kl32), kl32 = the fp32 KL mean.  The reference keeps the rate.  Taken (a) in the gradient call's
    prologue (grad_norm_ready, one rank: the runner's path) and (b) in the apply prologue from opt_state[8] planted as float64 values a
    quarter ulp either side of kl32 (what a float64 mean may be): every path keeps lr."""
    from hgym import make_ppo_config, make_batch
    S, B, lr = 5000, 4096, 1e-3
    p, net0, g, dims = _net("fused", B, 61, lr)
    cols = _batch_cols(p, dims, S, g)
    idx = torch.randperm(S, generator=g)[:B].contiguous().cuda()
    batch = make_batch(*cols, idx)
    net0.ppo_grad(make_ppo_config(adaptive=False), batch)
    torch.cuda.synchronize()
    kl32 = np.float32(float(net0.grads_ext[net0.P]))
    assert kl32 > 0
    desired = float(kl32 / np.float32(2)) if side == "upper" else float(kl32 * np.float32(2))
    assert reference_lr(lr, kl32, desired) == lr
    results = {}
    _, net, _, _ = _net("fused", B, 61, lr)
    ppo = make_ppo_config(desired_kl=desired, grad_norm_ready=True)
    net.ppo_grad(ppo, batch)
    net.ppo_apply(ppo)
    torch.cuda.synchronize()
    assert np.float32(float(net.grads_ext[net.P])) == kl32          # the same minibatch, the same KL
    results["gradient prologue"] = float(net.opt_state[L.OPT_LR])
    for q in (-0.25, 0.25):
        _, net, _, _ = _net("fused", B, 61, lr)
        ppo = make_ppo_config(desired_kl=desired, grad_norm_ready=False)
        net.ppo_grad(ppo, batch)
        net.opt_state[L.OPT_KL_LAST] = float(kl32) + q * float(np.spacing(kl32))
        net.ppo_apply(ppo)
        torch.cuda.synchronize()
        results["apply prologue, kl32 %+.2f ulp" % q] = float(net.opt_state[L.OPT_LR])
    assert all(v == lr for v in results.values()), results
