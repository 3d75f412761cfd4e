"""-m gpu: the action noise trained as log sigma (HgymNetConfig.std_param = HGYM_STD_LOG, ActorCritic(noise_std_type="log")).

The design makes the scalar mode the reference of the log mode: every kernel reads sigma through one pointer, which in log mode points at
a block the library derives (sigma = expf(log_std)), so a log net must compute, bit for bit, what a scalar net computes whose `std` holds
that block's values -- forward (2) and gradient (3), where the only difference allowed is the chain-rule product on the first A slots.
What the scalar mode cannot vouch for is checked on its own: the derived block (1), the gradient's formula against float64 autograd with
log_std as the leaf (4), the optimiser step on the log parameter (5), the diagnostics' reader (6) and the runner, captured and eager (7).

Paths: f32 (layer-by-layer, ppo_loss_kernel<float>), bf16-fused (ELU: mlp_fwd_kernel / mlp_fb_kernel), bf16-layer (nn.Tanh() without
fused_activation: gemm_nt_kernel in bf16, ppo_loss_kernel<bf16>)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16_report as BR
import loss_head_common as H
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu

XBOTL = (705, 219, [512, 256, 128], [768, 256, 128])
PATHS = {"f32": ("f32", None, False), "bf16-fused": ("bf16", None, True), "bf16-layer": ("bf16", nn.Tanh(), False)}
CASES = [("f32", 12), ("f32", 5), ("bf16-fused", 12), ("bf16-layer", 12)]       # A = 5: a 4-lane group of the head partly filled
IDS = ["%s-A%d" % c for c in CASES]
U = 2.0 ** -24
SUB = 8 * 2.0 ** -149


def _net(path, A, max_batch, noise_std_type, lr=1e-3):
    from hgym import NetBuffers, make_net_config
    precision, act, fused = PATHS[path]
    no, npv, ah, ch = XBOTL
    net = NetBuffers(make_net_config(no, npv, A, ah, ch, precision, max_batch, activation=act, noise_std_type=noise_std_type), "cuda",
                     learning_rate=lr)
    assert (net.shadow_ld(0) > 0) == fused, (path, net.shadow_ld(0))       # no row passes on another kernel
    return net


def _log_std(A):
    """several values in [-3, 1], in no order, none of them 0 (sigma = 1 would hide a reader that took the parameter for sigma less
    than the others do)"""
    v = -3.0 + 4.0 * (torch.arange(A, dtype=torch.float32) + 0.5) / A
    return v[torch.randperm(A, generator=torch.Generator().manual_seed(7))].contiguous()


def _pair(path, A, max_batch, seed):
    """(scalar net, log net, oracle params): the same weights; the log net's log_std planted, the scalar net's std := the log net's
    derived sigma, bit for bit."""
    g = torch.Generator().manual_seed(seed)
    no, npv, ah, ch = XBOTL
    p = P.Params.random(no, npv, A, ah, ch, g)
    b = _net(path, A, max_batch, "log")
    assert list(b.views)[0] == "log_std" and "std" not in b.views
    p.std = _log_std(A)
    b.load_state_dict(dict(zip(list(b.views), p.tensors())))
    sigma = b.sigma.clone()
    a = _net(path, A, max_batch, "scalar")
    assert list(a.views)[0] == "std" and a.sigma.data_ptr() == a.params.data_ptr()
    p.std = sigma.cpu()
    a.load_state_dict(dict(zip(list(a.views), p.tensors())))
    torch.cuda.synchronize()
    assert torch.equal(a.params[:A].view(torch.int32), b.sigma.view(torch.int32)) and torch.equal(a.params[A:], b.params[A:])
    assert bool((b.sigma > 0).all()) and not torch.equal(b.sigma, b.params[:A])
    return a, b, p, g


def _batch_cols(p, A, S, g):
    """S storage rows (tests/test_optimizer_step_gpu.py: _batch_cols, with p.std the standard deviations)"""
    no, npv = XBOTL[:2]
    obs, priv = torch.randn(S, no, generator=g), torch.randn(S, npv, generator=g)
    act, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = P.mlp_forward(obs, p.actor)
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    return [t.cuda().contiguous() for t in (obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o)]


# ---------------------------------------------------------------------------------------------- 1. sigma is derived and kept
@pytest.mark.parametrize("path", ["f32", "bf16-fused"])
def test_sigma_is_derived_and_kept(path):
    """sigma = expf(log_std) (sigma_of, hgym_net.hip) after hgym_net_sync_shadow: exactly 1 for 0; otherwise within 2 ulp of
    fp32(numpy.exp(float64(log_std))) -- HIP documents expf at 1 ulp, one more for the reference's own rounding to fp32.  After a
    hgym_ppo_apply the block adam_kernel left is, bit for bit, what hgym_net_sync_shadow derives from the new parameters."""
    from hgym import make_ppo_config
    A = 12
    net = _net(path, A, 64, "log")
    planted = np.array([0.0, math.log(0.05), math.log(4.0), -20.0, 3.0, -1.0, 1e-3, -1e-3, 0.5, -3.0, 1.0, -0.6931472], dtype=np.float32)
    assert not net.sigma.any()                                  # the zero fill, until the parameters are synchronised
    net.views["log_std"].copy_(torch.from_numpy(planted))
    net.sync_shadow()
    torch.cuda.synchronize()

    def ulps(sig, par):
        ref = np.exp(par.astype(np.float64)).astype(np.float32)
        return np.abs(sig.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref).astype(np.float64)

    got = net.sigma.cpu().numpy()
    assert got[0] == np.float32(1.0)
    worst = float(ulps(got, planted).max())
    print("\nsigma block %s after sync_shadow: worst %.2f ulp of fp32(exp64(log_std))" % (path, worst))
    assert worst <= 2.0, (got.tolist(), worst)
    assert bool((net.sigma > 0).all())
    # one optimiser step on an injected gradient: every log_std moves, and the block follows inside the Adam launch
    gd = torch.Generator(device="cuda").manual_seed(11)
    net.grads.copy_(torch.randn(net.P, device="cuda", generator=gd) * 1e-2)
    net.ppo_apply(make_ppo_config(adaptive=False))
    torch.cuda.synchronize()
    kept = net.sigma.clone()
    moved = net.params[:A].cpu().numpy()
    assert np.all(moved != planted) and not np.array_equal(kept.cpu().numpy(), got)
    assert float(ulps(kept.cpu().numpy(), moved).max()) <= 2.0
    net.sync_shadow()
    torch.cuda.synchronize()
    assert torch.equal(net.sigma.view(torch.int32), kept.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("path,A", CASES, ids=IDS)
def test_forward_is_bit_identical_to_the_scalar_mode(path, A):
    M = 33              # one 32-row tile plus a ragged row
    a, b, p, g = _pair(path, A, 64, 21)
    obs, priv, z = (torch.randn(M, n, generator=g).cuda() for n in (XBOTL[0], XBOTL[1], A))
    oa, ob = a.act(obs, priv, z=z), b.act(obs, priv, z=z)
    torch.cuda.synchronize()
    for k in ("actions", "mu", "sigma", "logp", "values"):
        assert torch.isfinite(ob[k]).all(), k
        assert torch.equal(oa[k], ob[k]), (path, A, k, float((oa[k] - ob[k]).abs().max()))
    assert torch.equal(ob["sigma"], b.sigma.expand(M, A))           # sigma itself, never its logarithm


# ---------------------------------------------------------------------------------------------- 3. gradient
@pytest.mark.parametrize("path,A", CASES, ids=IDS)
def test_gradient_is_the_scalar_one_times_sigma(path, A):
    """B = 65: one 64-row update tile plus one row.  Outside [0, A) the two gradients have the same bits; on [0, A) the log net's is
    fp32(scalar gradient) * sigma, one fp32 product; opt_state[HGYM_OPT_GRAD_SQNORM] is the squared norm of the gradient the log net
    returns (the bar of tests/test_optimizer_step_gpu.py::test_grad_norm_and_step_in_every_regime for the same quantity)."""
    from hgym import make_ppo_config, make_batch
    S, B = 80, 65
    a, b, p, g = _pair(path, A, 128, 31)
    cols = _batch_cols(p, A, S, g)
    idx = torch.randperm(S, generator=g)[:B].contiguous().cuda()
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config(adaptive=False)
    for net in (a, b):
        net.grads_ext.fill_(float("nan"))
        net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    ga, gb = a.grads_ext.clone(), b.grads_ext.clone()
    assert torch.isfinite(gb).all() and bool(ga[:A].ne(0).all())
    assert torch.equal(ga[A:].view(torch.int32), gb[A:].view(torch.int32))            # every weight, every bias, the KL slot
    assert torch.equal(gb[:A], ga[:A] * b.sigma), (gb[:A].tolist(), (ga[:A] * b.sigma).tolist())
    assert not torch.equal(gb[:A], ga[:A])
    for k in (L.OPT_SURROGATE_SUM, L.OPT_VALUE_SUM, L.OPT_ENTROPY_SUM, L.OPT_KL_LAST):
        assert float(a.opt_state[k]) == float(b.opt_state[k])
    G = b.grads.double().cpu().numpy()
    sq64 = math.fsum(G * G)
    nwg = 96 * len(b.views)
    bound = nwg * 2.0 ** -47 + (nwg + 128) * 2.0 ** -53 * sq64
    BR.check("log std %s A=%d: |opt[OPT_GRAD_SQNORM] - float64 sum over the returned gradient| / derived bound" % (path, A),
             abs(float(b.opt_state[L.OPT_GRAD_SQNORM]) - sq64) / bound, 1.0)
    # ... and NOT that of the scalar gradient (the product is in place before the norm is summed)
    Ga = a.grads.double().cpu().numpy()
    assert abs(math.fsum(Ga * Ga) - sq64) > 100 * bound


# ---------------------------------------------------------------------------------------------- 4. the formula
def _log_std_reference(rows, mu, v, sigma, ppo=H.PPO):
    """float64 autograd of the loss (ppo.py:128-168, as tests/loss_head_common.py::reference writes it out) with log_std the leaf:
    sigma = exp(log_std), log_std = log(sigma) of the standard deviations the kernels read.  -> d loss / d log_std, (A,)."""
    d = lambda t: torch.as_tensor(t).double()
    act, vold, adv, ret, lpo, mo, so = (d(rows[k]) for k in ("actions", "values", "adv", "returns", "logp", "mu_old", "sigma_old"))
    B, A = act.shape
    log_std = torch.log(d(sigma)).clone().requires_grad_()
    sig = torch.exp(log_std).expand(B, A)
    mu, v = d(mu), d(v)
    dist = torch.distributions.Normal(mu, sig)
    logp, ent = dist.log_prob(act).sum(-1), dist.entropy().sum(-1)
    ratio = torch.exp(logp - lpo)
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - ppo["clip"], 1.0 + ppo["clip"]))
    vc = vold + (v - vold).clamp(-ppo["clip"], ppo["clip"])
    vl = torch.max((v - ret).pow(2), (vc - ret).pow(2))
    loss = surr.mean() + ppo["value_coef"] * vl.mean() - ppo["entropy_coef"] * ent.mean()
    (g,) = torch.autograd.grad(loss, log_std)
    return g.detach()


@pytest.mark.parametrize("path", ["f32", "bf16-fused"])
def test_log_std_gradient_against_float64_autograd(path):
    """One strict case of the loss-head table's kind (B = 17, A = 12, shape xbotl) through the probe network, log_std = fp32(log std) of
    the case.  The reference is evaluated at the sigma the library derived (test 1 bounds that derivation on its own).  Bar per
    component: sigma_j x the bar tests/test_loss_head_gpu.py holds the std gradient to (sum_bar of the per-sample units at GPU_FACTOR *
    K_REF) + 2^-24 |ref_j| for the added product."""
    from hgym import make_ppo_config, make_batch
    case = H.make_case("bulk", 17, 12, "mid", 4242)
    assert not case["boundary"].any()
    n_obs, n_priv, ah, ch = H.SHAPES["xbotl"]
    net = _net(path, 12, 256, "log")
    p, obs_rows, priv_rows = H.probe_params(n_obs, n_priv, 12, ah, ch, case["mu"], case["v"], torch.log(case["std"]))
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    obs, priv = H.storage_inputs(case, n_obs, n_priv, obs_rows, priv_rows)
    c = case["cols"]
    cols = [t.cuda().contiguous() for t in (obs, priv, c["actions"], c["values"], c["adv"], c["returns"], c["logp"], c["mu_old"],
                                            c["sigma_old"])]
    batch = make_batch(*cols, case["idx"].cuda())
    net.grads_ext.fill_(float("nan"))
    net.ppo_grad(make_ppo_config(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.001), batch)
    torch.cuda.synchronize()
    sigma = net.sigma.cpu().double()
    assert float((sigma / case["std"].double() - 1).abs().max()) < 1e-6          # the case's std, to a few ulp: every sample stays strict
    got = net.grad_views()["log_std"].cpu().double()
    rows = H.rows_of(case)
    want = _log_std_reference(rows, case["mu"], case["v"], sigma)
    ref = H.reference(rows, case["mu"], case["v"], sigma)
    # (the two float64 routes agree, to float64 accuracy of the terms summed)
    assert bool(((want - ref["g_sigma"].sum(0) * sigma).abs() <= 1e-12 * ref["g_sigma"].abs().sum(0) * sigma).all())
    bar = sigma * H.sum_bar(H.units(ref)["g_sigma"], ref["g_sigma"], H.GPU_FACTOR * H.K_REF) + U * want.abs()
    r = ((got - want).abs() / bar).max()
    print("\nlog_std gradient %s: worst |kernel - float64 autograd| = %.3f x the bar; got %s want %s" % (path, float(r), got.tolist(),
                                                                                                      want.tolist()))
    assert torch.isfinite(got).all()
    BR.check("log_std gradient %s vs float64 autograd (log_std the leaf): worst err / bar" % path, float(r), 1.0)


# ---------------------------------------------------------------------------------------------- 5. the step
def _adam64(p_old, m_old, v_old, G, sq64, t, lr, max_norm, beta1, beta2, eps):
    """tests/test_optimizer_step_gpu.py::_adam64 restated: clip_grad_norm_ + one torch.optim.Adam step in float64 from the given state;
    returns (p, m, v, bounds p, m, v, coef).  Bounds, u = 2^-24: |m - m64| <= 8u (|beta1 m_old| + |(1 - beta1) g|); |v - v64| <= 16u v64
    (each + 8 x 2^-149); |p - p64| <= half an fp32 ulp of p + 16u |step64| + step_size x the m bound / denom64."""
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


@pytest.mark.parametrize("path", ["f32", "bf16-fused"])
def test_step_moves_log_std_by_clip_and_adam_on_the_returned_gradient(path):
    from hgym import make_ppo_config, make_batch
    A, S, B, lr = 12, 80, 65, 1e-3
    _, net, p, g = _pair(path, A, 128, 41)
    cols = _batch_cols(p, A, S, g)
    idx = torch.randperm(S, generator=g)[:B].contiguous().cuda()
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config(adaptive=False, grad_norm_ready=True)          # the runner's path: apply reuses the gradient call's norm
    state = lambda: [t.double().cpu().numpy() for t in (net.params, net.adam_m, net.adam_v)]
    before = state()
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    G = net.grads.double().cpu().numpy()
    sq64 = math.fsum(G * G)
    net.ppo_apply(ppo)
    torch.cuda.synchronize()
    after = state()
    p64, m64, v64, bp, bm, bv, coef = _adam64(*before, G, sq64, 1, lr, ppo.max_grad_norm, ppo.beta1, ppo.beta2, ppo.adam_eps)
    worst = 0.0
    for name, got, ref, bnd in (("params", after[0], p64, bp), ("adam_m", after[1], m64, bm), ("adam_v", after[2], v64, bv)):
        r_std, r_all = float((np.abs(got - ref) / bnd)[:A].max()), float((np.abs(got - ref) / bnd).max())
        assert r_std <= 1.0, "%s %s[:A]: worst |kernel - float64| / bound = %.3g (clip coefficient %.3g)" % (path, name, r_std, coef)
        assert r_all <= 1.0, "%s %s: worst |kernel - float64| / bound = %.3g" % (path, name, r_all)
        worst = max(worst, r_all)
    assert np.all(after[0][:A] != before[0][:A])
    BR.check("log std %s: clip + Adam on the returned gradient, worst err / derived bound" % path, worst, 1.0)
    # the block followed the step
    ref_sigma = np.exp(after[0][:A]).astype(np.float32)
    assert float((np.abs(net.sigma.cpu().numpy().astype(np.float64) - ref_sigma) / np.spacing(ref_sigma)).max()) <= 2.0


# ---------------------------------------------------------------------------------------------- 6. diagnostics
@pytest.mark.parametrize("path", ["f32", "bf16-fused"])
def test_diagnostics_read_sigma(path):
    """log_std = -1: a reader that took the parameter for sigma forms log(-1) = NaN."""
    import hgym
    from hgym import make_ppo_config
    M, A = 33, 12
    g = torch.Generator().manual_seed(51)
    no, npv, ah, ch = XBOTL
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.full((A,), -1.0)
    net = _net(path, A, 64, "log")
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    obs, priv, z = (torch.randn(M, n, generator=g).cuda() for n in (no, npv, A))
    out = net.act(obs, priv, z=z)
    ret, adv = torch.randn(M, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    cols = [obs, priv, out["actions"], out["values"].reshape(M).contiguous(), adv, ret, out["logp"], out["mu"], out["sigma"]]
    block = net.ppo_diagnostics(make_ppo_config(), cols, L.diag_block(M, "cuda"))
    torch.cuda.synchronize()
    d = hgym.diag_from_block(block)
    assert d["samples"] == M
    assert all(math.isfinite(float(d[k])) for k in hgym.DIAG_KEYS), d
    assert abs(d["kl"]) <= 1e-6, d["kl"]
    want = 12 * (0.5 + math.log(math.sqrt(2 * math.pi)) - 1.0)
    assert abs(d["entropy"] - want) <= 1e-6 * abs(want), (d["entropy"], want)


# ---------------------------------------------------------------------------------------------- 7. the runner
TASK = "humanoid_ppo"


def _runner(num_envs, seed):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    task_registry.train_cfgs[args.task].seed = seed
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


def _learn3(monkeypatch, graph, seen=None):
    """learn(3) at 64 envs with both graphs on or off -> the runner.  seen: receives the first rollout's sigma column and the net's
    sigma block as they stand before the first update."""
    monkeypatch.setenv("HGYM_GRAPH", graph)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", graph)
    torch.manual_seed(1357)
    np.random.seed(1357)
    r = _runner(64, 83)
    assert r.alg.actor_critic.noise_std_type == "log" and list(r.alg.net.views)[0] == "log_std"
    learn_step = r._learn_step

    def after_rollout(*a, **k):             # (learn() calls it between the rollout and the update; the first iteration runs eagerly)
        if seen is not None and not seen:
            seen.update(column=r.alg.storage.sigma.clone(), block=r.alg.net.sigma.clone())
        return learn_step(*a, **k)
    r._learn_step = after_rollout
    r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert (r._graph is not None) == (graph == "1") and (r._update_graph is not None) == (graph == "1")
    return r


def _finite_and_positive(r):
    net, st = r.alg.net, r.alg.storage
    assert torch.isfinite(net.params).all() and torch.isfinite(net.adam_m).all() and torch.isfinite(net.adam_v).all()
    assert torch.isfinite(net.opt_state).all()
    for name in ("actions", "mu", "sigma", "actions_log_prob", "values", "returns", "advantages"):
        assert torch.isfinite(getattr(st, name)).all(), name
    assert bool((net.sigma > 0).all()) and bool((st.sigma > 0).all())
    assert torch.equal(r.alg.actor_critic.noise_std, net.sigma)


def test_runner_trains_log_std_captured_as_eager(tmp_path, monkeypatch):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    PPO.precision = "bf16"
    pol = task_registry.train_cfgs[TASK].policy
    missing = object()
    keep = {k: getattr(pol, k, missing) for k in ("noise_std_type", "init_noise_std")}
    try:
        pol.noise_std_type = "log"
        seen = {}
        captured, eager = _learn3(monkeypatch, "1", seen), _learn3(monkeypatch, "0")
        for r in (captured, eager):
            _finite_and_positive(r)
        # the captured update keeps the sigma block current: three iterations, the same bits
        assert torch.equal(captured.alg.net.params.view(torch.int32), eager.alg.net.params.view(torch.int32))
        assert torch.equal(captured.alg.net.sigma.view(torch.int32), eager.alg.net.sigma.view(torch.int32))
        A = captured.alg.net.cfg.num_actions
        assert not torch.equal(captured.alg.net.sigma, seen["block"])                     # log_std has moved
        assert float(captured.alg.net.opt_state[L.OPT_STEP]) == 3 * 8
        # what the first rollout stored is sigma as it was before the first update: exp(log_std), the initial 1.0 here
        assert torch.equal(seen["column"], seen["block"].expand_as(seen["column"]))
        assert torch.equal(seen["block"], torch.ones(A, device="cuda"))
        path = str(tmp_path / "model_log.pt")
        captured.save(path)
        captured.wait_for_saves()
        ck = torch.load(path, map_location="cpu")
        assert list(ck["model_state_dict"])[:3] == ["log_std", "actor.0.weight", "actor.0.bias"] and "std" not in ck["model_state_dict"]
        assert torch.equal(ck["model_state_dict"]["log_std"], captured.alg.net.params[:A].cpu())
        # a small sigma (log_std = -4, sigma = 0.018) with the critic run once after the rollout
        pol.init_noise_std = math.exp(-4.0)
        monkeypatch.setenv("HGYM_ROLLOUT_CRITIC", "deferred")
        for graph in ("1", "0"):
            r = _learn3(monkeypatch, graph)
            _finite_and_positive(r)
            assert float(r.alg.net.sigma.max()) < 0.1
        monkeypatch.delenv("HGYM_ROLLOUT_CRITIC")
        # a policy of the other parametrisation refuses the file, and says which one the file has
        for k, v in keep.items():
            delattr(pol, k) if v is missing else setattr(pol, k, v)
        scalar = _runner(64, 83)
        assert scalar.alg.actor_critic.noise_std_type == "scalar"
        p0 = scalar.alg.net.params.clone()
        with pytest.raises(RuntimeError, match='noise_std_type="log"'):
            scalar.load(path)
        assert torch.equal(scalar.alg.net.params, p0)                                    # refused before anything was changed
        captured.load(path)                                                               # its own kind loads
    finally:
        for k, v in keep.items():
            if v is missing:
                if hasattr(pol, k):
                    delattr(pol, k)
            else:
                setattr(pol, k, v)
