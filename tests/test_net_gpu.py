"""-m gpu: actor/critic forward, PPO.act, and one full PPO iteration of libhgym_hip.so through the C-ABI against
(a) the golden vectors recorded from the reference and (b) the oracle on seeded inputs.

Tolerances: fp32 path <= 1e-5 relative (scale-relative for gradients); bf16 MFMA path <= 1e-2
relative, reported separately."""
import os

import numpy as np
import pytest
import torch

import bf16_report as BR
from oracle import ppo_oracle as P
from oracle import xbot_constants as K
from hgym import _lib as L

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.asarray(a))
NAMES = ["std"] + ["actor.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")] + \
        ["critic.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]


def _net(num_obs, num_priv, ah, ch, precision, max_batch, lr=1e-3, num_actions=12):
    from hgym import NetBuffers, make_net_config
    cfg = make_net_config(num_obs, num_priv, num_actions, ah, ch, precision, max_batch)
    return NetBuffers(cfg, "cuda", learning_rate=lr)


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


@pytest.mark.parametrize("precision,tol", [("f32", 1e-5), ("bf16", BR.BF16_BAR)])
def test_policy_example_known_answers(golden_dir, precision, tol):
    """The trained reference actor (logs/XBot_ppo/exported/policies/policy_example.pt) through the MFMA forward."""
    G = np.load(os.path.join(golden_dir, "policy_example.npz"))
    net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, precision, 4096)
    sd = {k: torch.zeros_like(v) for k, v in net.views.items()}
    for i in (0, 2, 4, 6):
        sd["actor.%d.weight" % i] = T(G["w_%d_weight" % i])
        sd["actor.%d.bias" % i] = T(G["w_%d_bias" % i])
    net.load_state_dict(sd)
    for x, y in ((torch.zeros(1, 705), G["y_zeros"]), (torch.linspace(-1, 1, 705)[None], G["y_linspace"]),
                 (T(G["x_rand"]), G["y_rand"])):
        out = net.forward(0, x.cuda().contiguous())
        torch.cuda.synchronize()
        err = _rel_err(out.cpu().numpy(), y)
        if precision == "bf16":
            BR.check("policy_example.pt actor forward, input %s" % (tuple(x.shape),), err, tol)
        assert err <= tol, (precision, err)
    # the literal SURVEY.md §8c numbers
    want0 = [0.08470258, -0.02338534, 0.00571555, 0.23484124, 0.63823998, -0.22751239, -0.11294249, -0.15007278,
             0.20418212, 0.35353008, 0.00772867, -0.45297036]
    out = net.forward(0, torch.zeros(1, 705, device="cuda")).cpu().numpy().ravel()
    assert _rel_err(out, want0) <= tol


@pytest.mark.parametrize("M", [1, 37, 128, 4096, 5000])
def test_forward_vs_oracle_f32(M):
    g = torch.Generator().manual_seed(M)
    p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
    net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, "f32", 5000)
    net.load_state_dict(dict(zip(NAMES, p.tensors())))
    obs = (torch.randn(M, 705, generator=g) * 2).clamp(-18, 18)
    priv = (torch.randn(M, 219, generator=g) * 2).clamp(-18, 18)
    mu = net.forward(0, obs.cuda())
    v = net.forward(1, priv.cuda())
    torch.cuda.synchronize()
    assert _rel_err(mu.cpu(), P.mlp_forward(obs, p.actor)) <= 1e-5
    assert _rel_err(v.cpu(), P.mlp_forward(priv, p.critic)) <= 1e-5


def test_policy_act_vs_oracle():
    g = torch.Generator().manual_seed(1)
    M = 300
    p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
    p.std = torch.rand(12, generator=g) + 0.5
    net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, "f32", M)
    net.load_state_dict(dict(zip(NAMES, p.tensors())))
    obs, priv, z = torch.randn(M, 705, generator=g), torch.randn(M, 219, generator=g), torch.randn(M, 12, generator=g)
    out = net.act(obs.cuda(), priv.cuda(), z=z.cuda())
    torch.cuda.synchronize()
    a, v, lp, mu, sg = P.policy_act(p, obs, priv, z)
    assert _rel_err(out["actions"].cpu(), a) <= 1e-5 and _rel_err(out["values"].cpu(), v) <= 1e-5
    assert _rel_err(out["mu"].cpu(), mu) <= 1e-5 and torch.equal(out["sigma"].cpu(), sg)
    np.testing.assert_allclose(out["logp"].cpu().numpy(), lp.numpy(), rtol=1e-5, atol=1e-4)
    # internal Philox sampling: right moments, reproducible for the same (seed, step), different across steps
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    o1 = net.act(obs.cuda(), priv.cuda(), seed=9, step_counter=step)["actions"].clone()
    o2 = net.act(obs.cuda(), priv.cuda(), seed=9, step_counter=step)["actions"].clone()
    step += 1
    o3 = net.act(obs.cuda(), priv.cuda(), seed=9, step_counter=step)["actions"].clone()
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)
    zz = ((o1.cpu() - mu) / sg).flatten()
    assert abs(float(zz.mean())) < 0.08 and abs(float(zz.std()) - 1.0) < 0.08
    # ... and at a sample size where the moments and the distribution itself can be held to 1e-2: 4096 rows x 12 actions x 8 steps
    # = 393 216 draws (standard error of the mean 1.6e-3, of the variance 2.3e-3; the 1 % critical value of the Kolmogorov-Smirnov
    # statistic at that size is 1.63 / sqrt(n) = 2.6e-3)
    g2 = torch.Generator().manual_seed(77)
    net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, "bf16", 4096)       # the rollout's own kernel (32-row tiles, bf16 operands)
    net.load_state_dict(dict(zip(NAMES, p.tensors())))
    obs2 = (torch.randn(4096, 705, generator=g2) * 2).clamp(-18, 18).cuda()
    priv2 = (torch.randn(4096, 219, generator=g2) * 2).clamp(-18, 18).cuda()
    zs = []
    for k in range(8):
        step.fill_(100 + k)
        o = net.act(obs2, priv2, seed=1234, step_counter=step)
        zs.append(((o["actions"] - o["mu"]) / o["sigma"]).double().flatten().cpu())
    z = torch.cat(zs)
    n = z.numel()
    assert abs(float(z.mean())) < 1e-2 and abs(float(z.var()) - 1.0) < 1e-2
    assert abs(float((z ** 3).mean())) < 2e-2 and abs(float((z ** 4).mean()) - 3.0) < 5e-2          # skewness 0, kurtosis 3
    zsort = torch.sort(z).values
    cdf = 0.5 * (1.0 + torch.erf(zsort / 2.0 ** 0.5))
    i = torch.arange(1, n + 1, dtype=torch.float64)
    ks = float(torch.maximum((i / n - cdf).abs().max(), (cdf - (i - 1) / n).abs().max()))
    assert ks < 1.63 / n ** 0.5 * 1.5, (ks, n)          # 1.5 x the 1 % critical value: fp32 draws, (a - mu) / sigma rounding
    assert float(z.abs().max()) > 4.0                   # the tails are there (P(|z| > 4) n = 25 draws expected)


def _run_iteration(G, precision):
    """Replays tests/golden/ppo_update.npz (or another recording of gen_fixtures.gen_ppo_update: ppo_update_arch.npz) from the reference's
    PPO through the HIP path."""
    from hgym import make_ppo_config, make_batch, _lib as L
    import ctypes as C
    Tn, N = G["obs"].shape[:2]
    A = G["z"].shape[-1]
    ah, ch = [int(x) for x in G["actor_hidden"]], [int(x) for x in G["critic_hidden"]]
    net = _net(G["obs"].shape[-1], G["priv"].shape[-1], ah, ch, precision, Tn * N, lr=1e-3, num_actions=A)
    net.load_state_dict({k: T(G["p0_" + k.replace(".", "_")]) for k in net.views})
    dev = "cuda"
    st = dict(obs=T(G["obs"]).to(dev).contiguous(), priv=T(G["priv"]).to(dev).contiguous())
    for k, shape in (("actions", (Tn, N, A)), ("mu", (Tn, N, A)), ("sigma", (Tn, N, A)), ("values", (Tn, N, 1)),
                     ("logp", (Tn, N)), ("rewards", (Tn, N)), ("returns", (Tn, N)), ("advantages", (Tn, N))):
        st[k] = torch.zeros(*shape, device=dev)
    dones = T(G["done"]).to(dev).to(torch.uint8).contiguous()
    s = net.stream()
    for t in range(Tn):
        out = dict(actions=st["actions"][t], mu=st["mu"][t], sigma=st["sigma"][t], logp=st["logp"][t], values=st["values"][t])
        net.act(st["obs"][t], st["priv"][t], z=T(G["z"][t]).to(dev).contiguous(), out=out)   # producers write the slot
        rew = T(G["rew_in"][t]).to(dev).contiguous()
        to = T(G["time_outs"][t]).to(dev).to(torch.uint8).contiguous()
        dslot = torch.zeros(N, dtype=torch.uint8, device=dev)
        L.check(L.lib.hgym_store_step(N, L.fptr(rew), L.fptr(st["values"][t]), L.u8ptr(to), L.u8ptr(dones[t]), 0.994,
                                      L.fptr(st["rewards"][t]), L.u8ptr(dslot), s))
    last_v = net.forward(1, T(G["last_priv"]).to(dev).contiguous()).view(N).contiguous()
    stats = L.gae_stats(N, dev)
    vals2d = st["values"].view(Tn, N)
    L.check(L.lib.hgym_gae(Tn, N, L.fptr(st["rewards"]), L.fptr(vals2d), L.u8ptr(dones), L.fptr(last_v), 0.994, 0.9,
                           L.fptr(st["returns"]), L.fptr(st["advantages"]), L.f64ptr(stats), s))
    L.check(L.lib.hgym_adv_normalize(Tn * N, L.fptr(st["advantages"]), L.f64ptr(stats), s))
    torch.cuda.synchronize()
    res = dict(net=net, st=st)
    ppo = make_ppo_config()
    perm = T(G["perm"]).to(dev)
    mb = perm.numel() // 4
    flat = {k: st[k].flatten(0, 1) if st[k].dim() > 2 else st[k].flatten() for k in st}
    lrs, g0 = [], None
    for epoch in range(2):
        for i in range(4):
            idx = perm[i * mb:(i + 1) * mb].contiguous()
            b = make_batch(flat["obs"], flat["priv"], flat["actions"], flat["values"].flatten(), flat["advantages"],
                           flat["returns"], flat["logp"], flat["mu"], flat["sigma"], idx)
            net.ppo_grad(ppo, b)
            net.ppo_apply(ppo)
            torch.cuda.synchronize()
            lrs.append(float(net.opt_state[L.OPT_LR]))
            if g0 is None:
                g0 = {k: v.clone().cpu() for k, v in net.grad_views().items()}
    res.update(lrs=lrs, g0=g0, opt=net.opt_state.cpu().clone())
    return res


def test_ppo_iteration_matches_reference_f32(golden_dir):
    _check_iteration_f32(np.load(os.path.join(golden_dir, "ppo_update.npz")))


def test_ppo_iteration_at_an_odd_architecture_matches_reference_f32(golden_dir):
    """tests/golden/ppo_update_arch.npz (gen_arch_fixture.py): actor [37, 5], critic [100, 17, 65, 3], 141 / 73 observations, 5 actions --
    the layer-by-layer path at 3 + 5 layers, ragged widths and a 5-wide head, against the reference's own iteration, at the bars above."""
    G = np.load(os.path.join(golden_dir, "ppo_update_arch.npz"))
    assert G["z"].shape[-1] == 5 and list(G["critic_hidden"]) == [100, 17, 65, 3]
    _check_iteration_f32(G)


def _check_iteration_f32(G):
    r = _run_iteration(G, "f32")
    names = list(r["net"].views)
    st = r["st"]
    for k, ref, tol in (("actions", G["actions"], 1e-5), ("values", G["values"], 1e-5), ("mu", G["mu"], 1e-5),
                        ("rewards", G["st_rewards"].squeeze(-1), 1e-5), ("returns", G["st_returns"].squeeze(-1), 1e-5),
                        ("advantages", G["st_advantages"].squeeze(-1), 1e-4)):
        assert _rel_err(st[k].cpu().numpy(), ref) <= tol, (k, _rel_err(st[k].cpu().numpy(), ref))
    np.testing.assert_allclose(st["logp"].cpu().numpy(), G["logp"], rtol=1e-5, atol=1e-4)
    # every adaptive-KL learning-rate decision identical to the reference's
    np.testing.assert_allclose(r["lrs"], G["lrs"], rtol=1e-12)
    # clipped gradients of the first minibatch vs the reference's autograd
    for k in names:
        ref = G["g0_" + k.replace(".", "_")]
        assert _rel_err(r["g0"][k].numpy(), ref) <= 5e-5, (k, _rel_err(r["g0"][k].numpy(), ref))
    # parameters after the 8 Adam steps
    for k in names:
        ref = G["pF_" + k.replace(".", "_")]
        np.testing.assert_allclose(r["net"].views[k].cpu().numpy(), ref, rtol=2e-4, atol=5e-6, err_msg=k)
    opt = r["opt"]
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]), float(G["mean_value_loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM] / opt[L.OPT_MINIBATCHES]), float(G["mean_surrogate_loss"]), rtol=1e-3, atol=1e-6)
    assert int(opt[L.OPT_STEP]) == 8 and int(opt[L.OPT_MINIBATCHES]) == 8


def test_ppo_iteration_bf16_close_to_reference(golden_dir):
    """bf16 MFMA path: reported separately with the 1e-2 class tolerance (gradient direction + parameter drift)."""
    G = np.load(os.path.join(golden_dir, "ppo_update.npz"))
    r = _run_iteration(G, "bf16")
    BR.check("ppo_update.npz (small net) rollout values", _rel_err(r["st"]["values"].cpu().numpy(), G["values"]))
    BR.check("ppo_update.npz (small net) rollout mu", _rel_err(r["st"]["mu"].cpu().numpy(), G["mu"]))
    num = den_a = den_b = 0.0
    for k in NAMES:
        a, b = r["g0"][k].double().flatten(), T(G["g0_" + k.replace(".", "_")]).double().flatten()
        num += float(a @ b); den_a += float(a @ a); den_b += float(b @ b)
    cos = num / (den_a ** 0.5 * den_b ** 0.5)
    assert cos > 0.995, cos
    assert r["lrs"][0] == G["lrs"][0]


def test_grad_vs_oracle_full_width():
    """Full XBot-L layer widths, ragged batch (not a tile multiple), fp32: un-clipped gradient vs the oracle."""
    from hgym import make_ppo_config, make_batch
    g = torch.Generator().manual_seed(3)
    S, B = 700, 333
    p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, "f32", 512)
    net.load_state_dict(dict(zip(NAMES, p.tensors())))
    obs, priv = torch.randn(S, 705, generator=g), torch.randn(S, 219, generator=g)
    act, mu_o = torch.randn(S, 12, generator=g), torch.randn(S, 12, generator=g) * 0.3
    sg_o = torch.rand(S, 12, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = P.mlp_forward(obs, p.actor)
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    out = P.ppo_loss_and_grads(p, obs[idx], priv[idx], act[idx], val[idx], adv[idx], ret[idx], lp_o[idx], mu_o[idx], sg_o[idx])
    c = lambda t: t.cuda().contiguous()
    keep = [c(obs), c(priv), c(act), c(val), c(adv), c(ret), c(lp_o), c(mu_o), c(sg_o), c(idx)]
    net.ppo_grad(make_ppo_config(), make_batch(*keep))
    torch.cuda.synchronize()
    gv = net.grad_views()
    for k, ref in zip(NAMES, out["grads"].tensors()):
        assert _rel_err(gv[k].cpu().numpy(), ref.numpy()) <= 5e-5, (k, _rel_err(gv[k].cpu().numpy(), ref.numpy()))
    opt = net.opt_state.cpu()
    np.testing.assert_allclose(float(opt[L.OPT_KL_LAST]), float(out["kl"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM]), float(out["value_loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM]), float(out["surrogate"]), rtol=1e-4, atol=1e-6)


FULL_SIZE_BF16_TOL = 5e-3      # fused kernels vs the bf16-operand oracle per tensor, rel-L2: the bound tests/test_fused_gpu.py holds at B = 4096


def test_update_full_size_vs_oracle():
    """BASELINE minibatch: B = 61 440 rows (960 tiles of 64 rows x 8 split-K slabs) gathered by a permutation out of a
    T * N = 245 760-row storage, XBot-L widths.  One minibatch through the fused bf16 kernels (mlp_fb_kernel, dw_kernel_rs, slab
    reduction) against the ORACLE's hand-written backward of /root/reference/humanoid/algo/ppo/ppo.py:128-174 evaluated on bf16
    operands (oracle/ppo_oracle.py: quant = bf16_round -- inputs, weights, activations and stored dZ rounded where the kernels
    round them, fp32 accumulation): per parameter tensor rel-L2 <= 5e-3, scalar losses within 1e-3.  The fp32 path on the same
    minibatch against the fp32 oracle: <= 1e-4 per tensor (accumulation order over 61 440 rows).  Then an Adam step moves the
    parameters."""
    from hgym import make_ppo_config, make_batch
    g = torch.Generator().manual_seed(11)
    S, B = 245760, 61440
    p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    dev = "cuda"
    gd = torch.Generator(device=dev).manual_seed(12)
    obs, priv = torch.randn(S, 705, device=dev, generator=gd).clamp_(-18, 18), torch.randn(S, 219, device=dev, generator=gd).clamp_(-18, 18)
    act, mu_o = torch.randn(S, 12, device=dev, generator=gd), torch.randn(S, 12, device=dev, generator=gd) * 0.3
    sg_o = torch.rand(S, 12, device=dev, generator=gd) * 0.5 + 0.75
    val, adv, ret = (torch.randn(S, device=dev, generator=gd) for _ in range(3))
    idx = torch.randperm(S, device=dev, generator=gd)[:B].contiguous()
    ic = idx.cpu()
    rows = lambda t: t[idx].cpu()
    o_obs, o_priv, o_act, o_mu, o_sg, o_val, o_adv, o_ret = (rows(t) for t in (obs, priv, act, mu_o, sg_o, val, adv, ret))
    # old log-probs near the current policy's (ratios around 1, both sides of the clip range populated)
    mu_now = P.mlp_forward(o_obs, p.actor)
    lp_rows = P.gaussian_log_prob(o_act, mu_now, mu_now * 0 + p.std) + torch.randn(B, generator=g) * 0.3
    lp_o = torch.zeros(S, device=dev)
    lp_o[idx] = lp_rows.to(dev)
    want = {None: P.ppo_loss_and_grads(p, o_obs, o_priv, o_act, o_val, o_adv, o_ret, lp_rows, o_mu, o_sg),
            "bf16": P.ppo_loss_and_grads(p, o_obs, o_priv, o_act, o_val, o_adv, o_ret, lp_rows, o_mu, o_sg, quant=P.bf16_round)}
    in_range = float(((want[None]["ratio"] > 0.8) & (want[None]["ratio"] < 1.2)).float().mean()) if "ratio" in want[None] else None
    rep = []
    for prec, ref, tol in (("f32", want[None], 1e-4), ("bf16", want["bf16"], FULL_SIZE_BF16_TOL)):
        net = _net(705, 219, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, prec, B)
        net.load_state_dict(dict(zip(NAMES, p.tensors())))
        net.ppo_grad(make_ppo_config(), make_batch(obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o, idx))
        torch.cuda.synchronize()
        assert torch.isfinite(net.grads).all()
        gv = net.grad_views()
        worst = 0.0
        for k, r in zip(NAMES, ref["grads"].tensors()):
            a, b = gv[k].cpu().double().flatten(), r.double().flatten()
            l2 = float((a - b).norm() / b.norm().clamp_min(1e-30))
            worst = max(worst, l2)
            assert l2 <= tol, (prec, k, l2)
        opt = net.opt_state.cpu()
        np.testing.assert_allclose(float(opt[L.OPT_KL_LAST]), float(ref["kl"]), rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM]), float(ref["value_loss"]), rtol=1e-3)
        np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM]), float(ref["surrogate"]), rtol=1e-3, atol=1e-5)
        rep.append("%s path vs %s oracle at B = %d: worst per-tensor rel-L2 %.3e (bound %.0e)" % (prec, "bf16-operand" if prec == "bf16" else "fp32", B, worst, tol))
        before = net.params.clone()
        net.ppo_apply(make_ppo_config())
        torch.cuda.synchronize()
        assert not torch.equal(before, net.params) and torch.isfinite(net.params).all()
        del net
    print("\n".join(rep), "| ratios inside the clip range:", in_range)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_apply_with_world_size_forms_the_rank_mean_itself(precision):
    """N>1 contract of hgym_ppo_apply: between grad and apply the ranks all-reduce (SUM) the P+1 floats of
    net.grads -- [flat gradient | minibatch KL] -- and apply divides by world_size on the device.  Emulated on one GPU:
    a net whose grads/KL slot hold world x the single-rank values, applied with world_size = world, must end bit-identical
    to the single-rank net (x2 and x0.5 are exact in fp32), including the adaptive-KL learning-rate step."""
    from hgym import NetBuffers, make_net_config, make_ppo_config
    world = 2
    nets = []
    for w in (1, world):
        torch.manual_seed(7)
        cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, 512)
        net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
        for k, v in net.views.items():
            v.copy_(torch.randn(v.shape, device="cuda") * 0.05)
        net.sync_shadow()
        g = torch.randn(net.P, device="cuda") * 3.0            # norm >> max_grad_norm: the clip is active
        net.grads.copy_(g * w)
        net.grads_ext[net.P] = 0.004 * w                        # mean KL 0.004 < desired_kl / 2 -> lr x 1.5
        net.opt_state[L.OPT_KL_LAST] = 123.0 if w > 1 else 0.004            # multi-rank: the local double is NOT what decides
        net.ppo_apply(make_ppo_config(world_size=w))
        torch.cuda.synchronize()
        nets.append(net)
    a, b = nets
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert float(a.opt_state[L.OPT_LR]) == float(b.opt_state[L.OPT_LR]) == pytest.approx(1.5e-3)
    assert float(a.opt_state[L.OPT_GRAD_NORM]) == float(b.opt_state[L.OPT_GRAD_NORM])       # same pre-clip gradient norm
    assert torch.equal(a.workspace, b.workspace)                # bf16 operand shadows follow


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_apply_can_reuse_the_norm_left_by_grad(precision):
    """HgymPPOConfig.grad_norm_ready: hgym_ppo_grad leaves the squared norm of its gradient in opt_state[9] (accumulated while the
    split-K slabs are summed); with the flag, hgym_ppo_apply skips its own pass over the gradient.  Both ways must agree: the
    norms to double rounding (different summation order), the updated parameters to 1e-7 relative."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    S = B = 1000
    nets = []
    for ready in (False, True):
        torch.manual_seed(11)
        cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, B)
        net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
        for k, v in net.views.items():
            v.copy_(torch.randn(v.shape, device="cuda") * (0.05 if v.dim() > 1 else 0.01))
        net.views["std"].fill_(1.0)
        net.sync_shadow()
        g = torch.Generator(device="cuda").manual_seed(5)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        cols = (r(S, 705), r(S, 219), r(S, 12), r(S), r(S) * 30.0, r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12, device="cuda"))
        idx = torch.randperm(S, device="cuda", generator=g).contiguous()
        ppo = make_ppo_config(grad_norm_ready=ready)
        assert ppo.grad_norm_ready == int(ready)
        net.ppo_grad(ppo, make_batch(*cols, idx))
        net.ppo_apply(ppo)
        torch.cuda.synchronize()
        nets.append(net)
    a, b = nets
    assert float(a.opt_state[L.OPT_GRAD_NORM]) > 1.0                         # the clip really acted (advantages x30)
    np.testing.assert_allclose(float(b.opt_state[L.OPT_GRAD_NORM]), float(a.opt_state[L.OPT_GRAD_NORM]), rtol=1e-6)
    np.testing.assert_allclose(b.params.cpu().numpy(), a.params.cpu().numpy(), rtol=1e-7, atol=1e-9)


def test_prologue_marker_keeps_grad_and_apply_in_step():
    """with grad_norm_ready on the fused one-rank path hgym_ppo_grad itself takes the adaptive-KL learning-rate decision and
    advances Adam's step count.  The marker in opt_state[13] keeps misuse from double-counting: (a) the normal sequence, (b) TWO gradient
    calls before one apply, (c) an apply under a configuration without the flag -- each must end with one optimiser step, one
    learning-rate decision and the same parameters (c: to the rounding of the norm it recomputes)."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    S = B = 1000
    res = {}
    for mode in ("normal", "grad twice", "apply without the flag"):
        torch.manual_seed(11)
        cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], "bf16", B)
        net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
        for k, v in net.views.items():
            v.copy_(torch.randn(v.shape, device="cuda") * (0.05 if v.dim() > 1 else 0.01))
        net.views["std"].fill_(1.0)
        net.sync_shadow()
        g = torch.Generator(device="cuda").manual_seed(5)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        cols = (r(S, 705), r(S, 219), r(S, 12), r(S), r(S), r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12, device="cuda"))
        idx = torch.randperm(S, device="cuda", generator=g).contiguous()
        ready = make_ppo_config(grad_norm_ready=True, desired_kl=0.01, adaptive=True)
        plain = make_ppo_config(grad_norm_ready=False, desired_kl=0.01, adaptive=True)
        for step in range(2):           # two optimiser steps: the marker must also be CLEARED by the apply
            net.ppo_grad(ready, make_batch(*cols, idx))
            if mode == "grad twice":
                net.ppo_grad(ready, make_batch(*cols, idx))
            net.ppo_apply(plain if mode == "apply without the flag" else ready)
        torch.cuda.synchronize()
        res[mode] = (net.params.clone(), net.opt_state.clone())
    lr0, steps0 = float(res["normal"][1][L.OPT_LR]), float(res["normal"][1][L.OPT_STEP])
    assert steps0 == 2.0 and lr0 != 1e-3
    for mode in ("grad twice", "apply without the flag"):
        o = res[mode][1]
        assert float(o[L.OPT_STEP]) == 2.0 and float(o[L.OPT_LR]) == lr0, (mode, o)
        np.testing.assert_allclose(res[mode][0].cpu().numpy(), res["normal"][0].cpu().numpy(), rtol=1e-6, atol=1e-8, err_msg=mode)
    assert float(res["normal"][1][L.OPT_PROLOGUE_STEP]) == -1.0                  # applied: nothing pending


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_grad_in_two_parts_is_the_whole_gradient(precision):
    """hgym_ppo_grad_part 0 then 1 (the data-parallel update's two gradient buckets) leaves net.grads and the KL slot exactly
    as hgym_ppo_grad does; after part 0 alone the actor bucket [0, split) is already final."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    S = B = 777
    torch.manual_seed(3)
    cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, B)
    net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
    for k, v in net.views.items():
        v.copy_(torch.randn(v.shape, device="cuda") * (0.05 if v.dim() > 1 else 0.01))
    net.views["std"].fill_(0.9)
    net.sync_shadow()
    r = lambda *s: torch.randn(*s, device="cuda")
    cols = (r(S, 705), r(S, 219), r(S, 12), r(S), r(S), r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12, device="cuda"))
    idx = torch.randperm(S, device="cuda").contiguous()
    ppo = make_ppo_config()
    split = net.bucket_split
    assert split == 12 + 705 * 512 + 512 + 512 * 256 + 256 + 256 * 128 + 128 + 128 * 12 + 12
    net.ppo_grad(ppo, make_batch(*cols, idx))
    torch.cuda.synchronize()
    whole = net.grads_ext.clone()
    net.grads_ext.fill_(float("nan"))
    net.ppo_grad_part(ppo, make_batch(*cols, idx), 0)
    torch.cuda.synchronize()
    if precision == "bf16":       # the layer-by-layer f32 path does everything in part 0
        # (the critic's head bias, the very last parameter, is a loss-side sum and already there; the rest of its bucket is not)
        assert torch.equal(net.grads_ext[:split], whole[:split]) and torch.isnan(net.grads_ext[split:net.P - 1]).all()
    net.ppo_grad_part(ppo, make_batch(*cols, idx), 1)
    torch.cuda.synchronize()
    assert torch.equal(net.grads_ext, whole)


def test_grad_in_two_parts_with_a_layer_by_layer_aux_head():
    """A fused bf16 trunk with an auxiliary head too wide for the fused kernels (it takes the layer-by-layer path): part 1 sums that
    head's split-K slabs with the split counts part 0 wrote them with, and both parts together equal hgym_ppo_grad."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    S = B = 777
    torch.manual_seed(4)
    cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], "bf16", B, aux_hidden=[512, 768, 768], aux_out=96,
                          aux_target_offset=219 - 96)
    net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
    for k, v in net.views.items():
        v.copy_(torch.randn(v.shape, device="cuda") * (0.05 if v.dim() > 1 else 0.01))
    net.views["std"].fill_(0.9)
    net.sync_shadow()
    r = lambda *s: torch.randn(*s, device="cuda")
    cols = (r(S, 705), r(S, 219), r(S, 12), r(S), r(S), r(S), r(S) - 12.0, r(S, 12) * 0.3, torch.ones(S, 12, device="cuda"))
    idx = torch.randperm(S, device="cuda").contiguous()
    ppo = make_ppo_config(aux_coef=0.5)
    net.ppo_grad(ppo, make_batch(*cols, idx))
    torch.cuda.synchronize()
    whole = net.grads_ext.clone()
    assert torch.isfinite(whole).all() and whole[net.bucket_split:].abs().sum() > 0
    net.grads_ext.fill_(float("nan"))
    net.ppo_grad_part(ppo, make_batch(*cols, idx), 0)
    net.ppo_grad_part(ppo, make_batch(*cols, idx), 1)
    torch.cuda.synchronize()
    assert torch.equal(net.grads_ext, whole)


# ---------------------------------------------------------------------------------------------- full-width reference fixture
def _full_case():
    import ppo_full_common as F
    G, p0, I = F.load()
    Gin = dict(I)
    Gin.update(actor_hidden=np.array(F.CASE.ACTOR_HIDDEN), critic_hidden=np.array(F.CASE.CRITIC_HIDDEN))
    Gin.update({"p0_" + k.replace(".", "_"): v for k, v in p0.items()})
    return F, G, p0, Gin


def test_ppo_iteration_full_width_matches_reference_f32():
    """tests/golden/ppo_update_full.npz: the reference's PPO (ppo.py:91-184) at the real layer widths 705-512-256-128-12 /
    219-768-256-128-1, 4 minibatches of 164 rows.  fp32 path: element-wise on the fp32-exact samples."""
    F, G, p0, Gin = _full_case()
    r = _run_iteration(Gin, "f32")
    st = r["st"]
    for k, ref, tol in (("actions", G["actions"], 1e-5), ("values", G["values"], 1e-5), ("mu", G["mu"], 1e-5),
                        ("rewards", G["st_rewards"].squeeze(-1), 1e-5), ("returns", G["st_returns"].squeeze(-1), 1e-5),
                        ("advantages", G["st_advantages"].squeeze(-1), 1e-4)):
        assert _rel_err(st[k].cpu().numpy(), ref) <= tol, (k, _rel_err(st[k].cpu().numpy(), ref))
    np.testing.assert_allclose(r["lrs"], G["lrs"], rtol=1e-12)
    rep = []
    for name, d in F.compare(G, "g0", {k: v.numpy() for k, v in r["g0"].items()}, rep).items():
        assert d["sample_max_err"] <= 5e-5 and abs(d["norm_ratio"] - 1) <= 2e-4, (name, d)
    dP = {k: r["net"].views[k].cpu().numpy() - p0[k] for k in NAMES}
    for name, d in F.compare(G, "dP", dP, rep).items():
        # Adam divides by sqrt(v): entries whose gradient is ~0 amplify fp32 summation-order differences, so the element-wise
        # bound on the parameter CHANGE is looser than on the gradient; the tensor as a whole agrees to 1e-3
        assert d["sample_max_err"] <= 2e-2 and d["rel_l2"] <= 1e-3 and abs(d["norm_ratio"] - 1) <= 2e-3, (name, d)
    print("\n".join(rep))
    opt = r["opt"]
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]), float(G["mean_value_loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM] / opt[L.OPT_MINIBATCHES]), float(G["mean_surrogate_loss"]), rtol=1e-3, atol=1e-6)


# per-tensor tolerance of the bf16 FUSED path against the reference's fp32 autograd, first-minibatch clipped gradient (measured:
# profiles/r02_bf16_full_width_parity.txt); rel-L2 error | cosine
BF16_G0_TOL = {"rel_l2": 2e-2, "cos": 0.9997}      # measured: rel-L2 1.8e-3 .. 7.7e-3, cosine >= 0.99997
# ... and of the 8-step parameter change, per tensor
BF16_DP_TOL = {"rel_l2": 8e-2, "cos": 0.997, "norm": 5e-3}


def test_ppo_iteration_full_width_bf16_fused_kernels_vs_reference(capsys):
    """The same fixture through the kernels bench.py times: mlp_fwd_kernel<32,8,4> (rollout, 82 rows = two 32-row tiles + a
    ragged one), mlp_fb_kernel (forward + PPO loss + dZ chain in one launch) / dw_kernel_rs (update, 164 rows = two 64-row tiles + a ragged one).
    bf16 operands, fp32 accumulation: activations within 2e-2, first learning-rate decision identical, the clipped gradient of
    the first minibatch within BF16_G0_TOL per tensor, the 8-step parameter change in the same direction."""
    from hgym import _lib as L
    F, G, p0, Gin = _full_case()
    L.lib.hgym_prof_enable(1)
    r = _run_iteration(Gin, "bf16")
    fused = [L.prof_summary(c)[0] for c in (L.PROF_POLICY, L.PROF_MLP_FWD, L.PROF_MLP_BWD, L.PROF_DW)]
    generic = L.prof_summary(L.PROF_GEMM)[0]
    L.lib.hgym_prof_enable(0)
    # the fused kernels ran: T rollout steps + bootstrap; per minibatch ONE forward + loss + dZ-chain launch (mlp_fb_kernel, counted
    # in the forward class; the stand-alone dZ-chain kernel no longer runs) and one weight-gradient launch ...
    assert fused[0] >= F.CASE.T and fused[1:] == [8, 0, 8], fused
    assert generic == 0                                                 # ... and no layer-by-layer GEMM did
    st = r["st"]
    BR.check("ppo_update_full.npz (real widths) rollout values", _rel_err(st["values"].cpu().numpy(), G["values"]))
    BR.check("ppo_update_full.npz (real widths) rollout mu", _rel_err(st["mu"].cpu().numpy(), G["mu"]))
    BR.check("ppo_update_full.npz (real widths) returns", _rel_err(st["returns"].cpu().numpy(), G["st_returns"].squeeze(-1)))
    np.testing.assert_allclose(r["lrs"], G["lrs"], rtol=1e-12)       # all 8 adaptive-KL decisions as the reference took them
    rep = ["bf16 fused path vs reference fp32, clipped gradient of minibatch 0:"]
    cmp_g = F.compare(G, "g0", {k: v.numpy() for k, v in r["g0"].items()}, rep)
    rep.append("total cosine %.6f" % F.total_cosine(G, "g0", {k: v.numpy() for k, v in r["g0"].items()}))
    dP = {k: r["net"].views[k].cpu().numpy() - p0[k] for k in NAMES}
    rep.append("parameter change over 8 Adam steps:")
    cmp_p = F.compare(G, "dP", dP, rep)
    rep.append("total cosine %.6f ; lrs %s vs %s" % (F.total_cosine(G, "dP", dP), r["lrs"], list(G["lrs"])))
    with capsys.disabled():
        print("\n" + "\n".join(rep))
    for name, d in cmp_g.items():
        if name == "std":
            continue       # 12 numbers, each a sum over the batch of a difference of O(1) terms: compared in absolute terms below
        assert d["rel_l2"] <= BF16_G0_TOL["rel_l2"] and d["cos"] >= BF16_G0_TOL["cos"], (name, d)
    assert F.total_cosine(G, "g0", {k: v.numpy() for k, v in r["g0"].items()}) >= 0.999
    assert F.total_cosine(G, "dP", dP) >= 0.995                     # measured 0.9986
    # per tensor (measured, profiles/r02_bf16_full_width_parity.txt: rel-L2 <= 5.9e-2, cosine >= 0.99828, norm ratio within 2.7e-3).
    # An Adam step is lr * m / (sqrt(v) + eps) ~ lr * sign(g) for the first steps: an entry whose gradient is within the bf16
    # error of zero moves by the full step in the other direction, so single ENTRIES differ by up to 2 steps (sample_max_err ~ 1)
    # while every tensor as a whole keeps its direction and length -- that is the statement asserted.
    for name, d in cmp_p.items():
        assert d["rel_l2"] <= BF16_DP_TOL["rel_l2"] and d["cos"] >= BF16_DP_TOL["cos"] and abs(d["norm_ratio"] - 1) <= BF16_DP_TOL["norm"], (name, d)


def test_norm_pass_of_apply_is_one_launch_and_reproducible():
    """hgym_ppo_apply's own norm pass (several ranks / foreign gradients): per-workgroup fp64 partial sums added in a fixed order by the last
    workgroup to arrive, which also takes the prologue (sqnorm_prologue_kernel) -- no atomics on the sum.  The same state applied five times
    gives the same bits (norm, learning rate, parameters); the norm is the fp64 norm of the rank mean to 1e-12; the arrival counter is left
    at zero, so a second apply on the same net works."""
    from hgym import NetBuffers, make_net_config, make_ppo_config
    outs = []
    for rep in range(5):
        torch.manual_seed(3)
        cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], "bf16", 512)
        net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
        for k, v in net.views.items():
            v.copy_(torch.randn(v.shape, device="cuda") * 0.05)
        net.sync_shadow()
        g = torch.randn(net.P, device="cuda") * 3.0
        net.grads.copy_(g)
        net.grads_ext[net.P] = 0.02
        net.ppo_apply(make_ppo_config(world_size=4))
        torch.cuda.synchronize()
        want = float((g.double() * float(np.float32(0.25))).pow(2).sum().sqrt())
        assert abs(float(net.opt_state[L.OPT_GRAD_NORM]) - float(np.float32(want))) <= 1e-6 * want       # opt[6] = the fp32 norm the clip used
        assert abs(float(net.opt_state[L.OPT_GRAD_SQNORM]) - want * want) <= 1e-12 * want * want
        outs.append((net.opt_state.clone(), net.params.clone(), net.adam_v.clone()))
        if rep == 0:                                  # a second step on the same net: the counter was reset
            net.grads.copy_(g)
            net.grads_ext[net.P] = 0.02
            net.ppo_apply(make_ppo_config(world_size=4))
            torch.cuda.synchronize()
            assert int(net.opt_state[L.OPT_STEP]) == 2 and torch.isfinite(net.params).all()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
