"""-m gpu: the unclipped value loss (HgymPPOConfig.value_loss_unclipped = 1, the reference's use_clipped_value_loss = False) through
every update path, against a float64 autograd restatement of (R - V)^2.mean(), against the reference's own PPO
(tests/golden/ppo_update_unclipped.npz, ppo_update_full_unclipped.npz: gen_value_loss_fixtures.py), and end to end in the runner.

Kernel level: the stored old values are moved by +-0.5 against clip = 0.2, so that about half of the rows lie outside the clip range;
there the two forms give different critic gradients (the clipped form drops the row), which shows that the flag reaches the kernel."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import bf16_report as BR
from oracle import ppo_oracle as P

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5                                 # fp32 gradient, per tensor, worst element / largest element (measured <= 3.9e-7)
BF16_TOL = {"rel_l2": 2e-2, "cos": 0.9997}     # bf16 gradient, per tensor (test_net_gpu.py: BF16_G0_TOL)
S, B = 5000, 4096
XBOTL = ([512, 256, 128], [768, 256, 128])
PATHS = {      # name: (actor hidden, critic hidden, precision, activation, aux (hidden, outputs) or None, fused)
    "f32-gemm": (*XBOTL, "f32", None, None, False),
    "bf16-gemm-tanh": (*XBOTL, "bf16", nn.Tanh(), None, False),
    "bf16-gemm-wide-actor": ([768, 256, 128], [768, 256, 128], "bf16", None, None, False),   # the actor does not fit the fused tile
    "bf16-fused-xbotl": (*XBOTL, "bf16", None, None, True),                       # the `pre` loss-input gather on
    "bf16-fused-256x3": ([256, 256, 256], [256, 256, 256], "bf16", None, None, True),   # third width 256: `pre` off
    "bf16-fused-denoiser": (*XBOTL, "bf16", None, ([512, 256, 256], 73), True),   # + the auxiliary head's grid row
}


def _critic_names():
    return ["critic.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]


def _reference(p, act, priv, ret, coef):
    """float64 autograd of coef * (R - V)^2.mean() with respect to the critic's parameters; returns (gradients, (R - V)^2.mean())."""
    f = act if act is not None else nn.ELU()
    layers = [(W.double().requires_grad_(), b.double().requires_grad_()) for W, b in p.critic]
    h = priv.double()
    for i, (W, b) in enumerate(layers):
        h = Fn.linear(h, W, b)
        if i < len(layers) - 1:
            h = f(h)
    vl = (ret.double() - h.squeeze(-1)).pow(2).mean()
    (coef * vl).backward()
    return [t.grad for W, b in layers for t in (W, b)], float(vl)


def _setup(name):
    from hgym import NetBuffers, make_net_config
    ah, ch, precision, act, aux, fused = PATHS[name]
    g = torch.Generator().manual_seed(31)
    p = P.Params.random(705, 219, 12, ah, ch, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    kw = dict(aux_hidden=aux[0], aux_out=aux[1], aux_target_offset=219 - aux[1]) if aux else {}
    net = NetBuffers(make_net_config(705, 219, 12, ah, ch, precision, S, activation=act, **kw), "cuda", learning_rate=1e-3)
    sd = dict(zip(list(net.views), p.tensors()))
    if aux:
        head = P.Params.random(705, 219, aux[1], aux[0], [8, 8, 8], g).actor
        for l, (W, b) in enumerate(head):
            sd["denoiser.%d.weight" % (2 * l)], sd["denoiser.%d.bias" % (2 * l)] = W, b
    net.load_state_dict(sd)
    assert (net.shadow_ld(0) > 0 and net.shadow_ld(1) > 0) == fused
    return p, net, g


def _ppo_grad_rc(net, ppo, batch):
    from hgym import _lib as L
    return int(L.lib.hgym_ppo_grad(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(batch), net.stream()))


@pytest.mark.parametrize("name", list(PATHS))
def test_one_minibatch_on_every_path(name):
    from hgym import _lib as L, make_ppo_config, make_batch
    ah, ch, precision, act, aux, fused = PATHS[name]
    p, net, g = _setup(name)
    obs, priv = torch.randn(S, 705, generator=g), torch.randn(S, 219, generator=g)
    actions, mu_o = torch.randn(S, 12, generator=g), torch.randn(S, 12, generator=g) * 0.3
    sg_o = torch.rand(S, 12, generator=g) * 0.5 + 0.75
    adv = torch.randn(S, generator=g)
    ret = torch.randn(S, generator=g) * 0.5 + 1.0            # away from V ~ 0: the last bias' gradient is not a cancelling sum
    with torch.no_grad():
        mu_now = net.forward(0, obs.cuda()).cpu()
        v_now = net.forward(1, priv.cuda()).cpu().view(S)
    lp_o = P.gaussian_log_prob(actions, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    vold = v_now + torch.where(torch.rand(S, generator=g) < 0.5, 0.5, -0.5)     # |V - V_old| = 0.5 > clip = 0.2 on every row
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    cols = [t.cuda().contiguous() for t in (obs, priv, actions, vold, adv, ret, lp_o, mu_o, sg_o)] + [idx.cuda()]
    batch = make_batch(*cols)
    coef = 0.7
    aux_coef = 0.5 if aux else 0.0
    unclipped = make_ppo_config(value_loss_coef=coef, aux_coef=aux_coef, clipped_value_loss=False)
    clipped = make_ppo_config(value_loss_coef=coef, aux_coef=aux_coef)
    # the clipped form with a zero-filled tail: the layout every caller before the field had
    tail = L.PPOConfig()
    C.memmove(C.addressof(tail), C.addressof(clipped), L.PPOConfig.value_loss_unclipped.offset)
    opt0 = net.opt_state.clone()

    def run(ppo):
        net.opt_state.copy_(opt0)
        net.grads_ext.zero_()
        net.ppo_grad(ppo, batch)
        torch.cuda.synchronize()
        return net.grads_ext.clone(), net.opt_state.clone()

    L.lib.hgym_prof_enable(1)
    g_u, o_u = run(unclipped)
    counts = {c: L.prof_summary(c)[0] for c in (L.PROF_GEMM, L.PROF_LOSS, L.PROF_MLP_FWD)}
    L.lib.hgym_prof_enable(0)
    if fused:       # one mlp_fb_kernel launch, no layer-by-layer GEMM
        assert counts[L.PROF_MLP_FWD] >= 1 and counts[L.PROF_GEMM] == 0, counts
    else:           # the layer-by-layer GEMMs and ppo_loss_kernel
        assert counts[L.PROF_GEMM] > 0 and counts[L.PROF_LOSS] == 1, counts
    g_c, o_c = run(clipped)
    g_t, _ = run(tail)
    assert torch.equal(g_t, g_c)                       # zero-filled tail = explicit 0

    # the critic's gradient against the restated unclipped loss
    sel = idx.long()
    want, vl = _reference(p, act, priv[sel], ret[sel], coef)
    off_c, off_x = net.bucket_split, int(L.lib.hgym_net_param_offset(C.byref(net.cfg), 2))
    report = []
    worst_u = 0.0
    for k, w in zip(_critic_names(), want):
        v = net.views[k]
        o = (v.data_ptr() - net.params.data_ptr()) // 4
        got = g_u[o:o + v.numel()].view_as(v).cpu().double()
        if precision == "f32":
            err = float((got - w).abs().max() / w.abs().max())
            assert err <= F32_TOL, (k, err)
            report.append("%s: %.2e (bar %.0e)" % (k, err, F32_TOL))
            worst_u = max(worst_u, err)
        else:
            a, b = got.flatten(), w.flatten()
            rel = float((a - b).norm() / b.norm())
            cos = float(a @ b / (a.norm() * b.norm()))
            BR.check("unclipped value loss, %s, %s gradient vs float64 autograd, rel-L2" % (name, k), rel, BF16_TOL["rel_l2"])
            BR.check("unclipped value loss, %s, %s gradient vs float64 autograd, 1 - cosine" % (name, k), 1.0 - cos, 1.0 - BF16_TOL["cos"])
            worst_u = max(worst_u, rel)
    print("\n%s, unclipped critic gradient vs float64 autograd: %s" % (name, "; ".join(report) if report else "worst rel-L2 %.2e" % worst_u))
    if precision == "f32":
        assert abs(float(o_u[4]) - vl) <= 1e-5 * vl, (float(o_u[4]), vl)
    # the clipped form is far from it: the flag reached the kernel
    cu, cc = g_u[off_c:off_x].double(), g_c[off_c:off_x].double()
    sep = float((cc - cu).norm() / cu.norm())
    bar = F32_TOL if precision == "f32" else BF16_TOL["rel_l2"]
    print("%s: clipped vs unclipped critic gradient, rel-L2 %.3e (must be >= %.1e)" % (name, sep, 10 * bar))
    assert sep >= 10 * bar, sep
    assert float(o_u[4]) != float(o_c[4])
    # std, actor, auxiliary head: bit-identical; so are the other loss sums
    assert torch.equal(g_u[:off_c], g_c[:off_c])
    assert torch.equal(g_u[off_x:], g_c[off_x:])       # the auxiliary head (if any) and the KL slot
    assert torch.equal(o_u[[2, 3, 5, 8, 10]], o_c[[2, 3, 5, 8, 10]])

    # any other value of the field is refused, before anything runs
    for bad in (2, -1):
        cfg = make_ppo_config(clipped_value_loss=False)
        cfg.value_loss_unclipped = bad
        assert _ppo_grad_rc(net, cfg, batch) == -1                  # HGYM_E_BADARG
        assert b"value_loss_unclipped" in L.lib.hgym_last_error()
        assert int(L.lib.hgym_ppo_apply(C.byref(net.cfg), C.byref(cfg), C.byref(net.struct), net.stream())) == -1
        assert int(L.lib.hgym_ppo_grad_part(C.byref(net.cfg), C.byref(cfg), C.byref(net.struct), C.byref(batch), 0, net.stream())) == -1


# ---------------------------------------------------------------------------------------------- the reference's PPO, unclipped
# The unclipped fixtures hold the update's results only (tests/golden/value_loss_case.py): the replay runs on the clipped fixtures' inputs,
# and gradients / parameters are compared on the fp32-exact samples the fixtures keep, at the bounds of the clipped replays in
# tests/test_net_gpu.py (rel-L2 and cosine over the sample; the norm ratio against the full tensor's recorded norm).
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import value_loss_case as V  # noqa: E402
from hgym import _lib as L

# rel-L2 distance between the unclipped and the clipped fixture's 8-step parameter change, as gen_value_loss_fixtures.py prints it, of
# the tensors where it is at least 10x the bar the replay is held to (fp32 dP: 1e-3): only those can show which form the replay took
SEPARATION_SMALL = ["critic.0.weight", "critic.2.weight", "critic.4.weight", "critic.6.weight"]    # 1.2e-1, 1.4e-1, 7.7e-2, 5.8e-2
SEPARATION_FULL = {"critic.0.weight": 2.00e-1, "critic.2.weight": 1.58e-1, "critic.4.weight": 7.59e-2, "critic.6.weight": 5.35e-2,
                   "critic.4.bias": 9.81e-2, "critic.6.bias": 1.01e-1}


def _load(name):
    U = np.load(os.path.join(GOLDEN, name))
    assert not bool(U["use_clipped_value_loss"])
    return U


def _unclipped_iteration(monkeypatch, G, precision):
    """tests/test_net_gpu.py's replay of a recorded PPO iteration, with every PPO configuration it makes unclipped."""
    import hgym
    import test_net_gpu as NG
    monkeypatch.setattr(hgym, "make_ppo_config", functools.partial(hgym.make_ppo_config, clipped_value_loss=False))
    return NG._run_iteration(G, precision)


def _compare_samples(U, prefix, got, report):
    """got: name -> full fp32 tensor; per tensor, the entries at value_loss_case.sample_index against the fixture's samples."""
    out = {}
    for name in V.NAMES:
        key = name.replace(".", "_")
        a = np.asarray(got[name], dtype=np.float64).reshape(-1)
        x, s = a[V.sample_index(name, a.size, prefix)], U["%s_s32_%s" % (prefix, key)].astype(np.float64)
        d = dict(rel_l2=float(np.linalg.norm(x - s) / max(np.linalg.norm(s), 1e-30)),
                 cos=float(x @ s / max(np.linalg.norm(x) * np.linalg.norm(s), 1e-30)),
                 sample_max_err=float(np.abs(x - s).max() / max(np.abs(s).max(), 1e-30)),
                 norm_ratio=float(np.linalg.norm(a) / max(float(U["%s_norm_%s" % (prefix, key)]), 1e-30)))
        out[name] = d
        report.append("%s %-16s rel_l2 %.3e  cos %.6f  sample_max_err %.3e  |got|/|ref| %.4f" % (
            prefix, name, d["rel_l2"], d["cos"], d["sample_max_err"], d["norm_ratio"]))
    return out


def test_ppo_iteration_unclipped_matches_reference_f32(monkeypatch):
    """ppo_update_unclipped.npz on the fp32 path, on ppo_update.npz's inputs, at test_net_gpu.py::test_ppo_iteration_matches_reference_f32's
    bounds."""
    import test_net_gpu as NG
    Cl = np.load(os.path.join(GOLDEN, "ppo_update.npz"))
    U = _load("ppo_update_unclipped.npz")
    r = _unclipped_iteration(monkeypatch, Cl, "f32")
    np.testing.assert_allclose(r["lrs"], U["lrs"], rtol=1e-12)
    for k in NG.NAMES:
        key = k.replace(".", "_")
        g = r["g0"][k].numpy().reshape(-1)
        ref = U["g0_s32_" + key]
        assert NG._rel_err(g[V.sample_index(k, g.size, "g0")], ref) <= 5e-5, (k, NG._rel_err(g[V.sample_index(k, g.size, "g0")], ref))
        pf = r["net"].views[k].cpu().numpy().reshape(-1)
        np.testing.assert_allclose(pf[V.sample_index(k, pf.size, "pF")], U["pF_s32_" + key], rtol=2e-4, atol=5e-6, err_msg=k)
    opt = r["opt"]
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]), float(U["mean_value_loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM] / opt[L.OPT_MINIBATCHES]), float(U["mean_surrogate_loss"]), rtol=1e-3, atol=1e-6)
    # the clipped fixture is out of reach: its mean value loss, and the parameter change of the separated tensors
    assert abs(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]) - float(Cl["mean_value_loss"])) > 10 * 1e-4 * float(Cl["mean_value_loss"])
    for k in SEPARATION_SMALL:
        key = k.replace(".", "_")
        pf = r["net"].views[k].cpu().numpy().reshape(-1).astype(np.float64)
        idx = V.sample_index(k, pf.size, "pF")
        p0 = Cl["p0_" + key].reshape(-1)[idx].astype(np.float64)
        got, ref_u = pf[idx] - p0, U["pF_s32_" + key].astype(np.float64) - p0
        ref_c = Cl["pF_" + key].reshape(-1)[idx].astype(np.float64) - p0
        d = np.linalg.norm(ref_u - ref_c) / np.linalg.norm(ref_c)       # what the fixtures themselves tell apart, on the kept entries
        e_u = np.linalg.norm(got - ref_u) / np.linalg.norm(ref_u)
        e_c = np.linalg.norm(got - ref_c) / np.linalg.norm(ref_c)
        assert d >= 10 * 1e-3 and e_c >= 0.5 * d and e_c >= 10 * e_u, (k, d, e_u, e_c)


def _full():
    import test_net_gpu as NG
    F, _, p0, Gin = NG._full_case()
    return NG, F, p0, Gin, _load("ppo_update_full_unclipped.npz")


def test_ppo_iteration_full_width_unclipped_f32(monkeypatch):
    """ppo_update_full_unclipped.npz on the fp32 path, at test_ppo_iteration_full_width_matches_reference_f32's bounds."""
    NG, F, p0, Gin, U = _full()
    r = _unclipped_iteration(monkeypatch, Gin, "f32")
    np.testing.assert_allclose(r["lrs"], U["lrs"], rtol=1e-12)
    rep = []
    for name, d in _compare_samples(U, "g0", {k: v.numpy() for k, v in r["g0"].items()}, rep).items():
        assert d["sample_max_err"] <= 5e-5 and abs(d["norm_ratio"] - 1) <= 2e-4, (name, d)
    dP = {k: r["net"].views[k].cpu().numpy() - p0[k] for k in NG.NAMES}
    for name, d in _compare_samples(U, "dP", dP, rep).items():
        assert d["sample_max_err"] <= 2e-2 and d["rel_l2"] <= 1e-3 and abs(d["norm_ratio"] - 1) <= 2e-3, (name, d)
    print("\n".join(rep))
    opt = r["opt"]
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]), float(U["mean_value_loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM] / opt[L.OPT_MINIBATCHES]), float(U["mean_surrogate_loss"]), rtol=1e-3, atol=1e-6)
    # ... and away from the clipped fixture (its full fp16 copy of dP), where the recorded distance allows telling them apart
    Cl = np.load(os.path.join(GOLDEN, "ppo_update_full.npz"))
    cmp_c = F.compare(Cl, "dP", dP)
    for k, d in SEPARATION_FULL.items():
        assert cmp_c[k]["rel_l2"] >= 0.5 * d, (k, cmp_c[k])
    assert abs(float(opt[L.OPT_VALUE_SUM] / opt[L.OPT_MINIBATCHES]) - float(Cl["mean_value_loss"])) > 10 * 1e-4 * float(Cl["mean_value_loss"])


def test_ppo_iteration_full_width_unclipped_bf16_fused(monkeypatch, capsys):
    """ppo_update_full_unclipped.npz through the fused bf16 kernels (mlp_fb_kernel<.., VU>), at
    test_ppo_iteration_full_width_bf16_fused_kernels_vs_reference's per-tensor bounds; the profiler shows that no layer-by-layer GEMM ran."""
    from hgym import _lib as L
    NG, F, p0, Gin, U = _full()
    L.lib.hgym_prof_enable(1)
    r = _unclipped_iteration(monkeypatch, Gin, "bf16")
    fused = [L.prof_summary(c)[0] for c in (L.PROF_POLICY, L.PROF_MLP_FWD, L.PROF_MLP_BWD, L.PROF_DW)]
    generic = L.prof_summary(L.PROF_GEMM)[0]
    L.lib.hgym_prof_enable(0)
    assert fused[0] >= F.CASE.T and fused[1:] == [8, 0, 8], fused
    assert generic == 0
    np.testing.assert_allclose(r["lrs"], U["lrs"], rtol=1e-12)
    rep = ["bf16 fused path vs reference fp32, unclipped value loss (fixture samples):"]
    cmp_g = _compare_samples(U, "g0", {k: v.numpy() for k, v in r["g0"].items()}, rep)
    dP = {k: r["net"].views[k].cpu().numpy() - p0[k] for k in NG.NAMES}
    cmp_p = _compare_samples(U, "dP", dP, rep)
    with capsys.disabled():
        print("\n" + "\n".join(rep))
    for name, d in cmp_g.items():
        if name == "std":
            continue       # 12 numbers, each a sum over the batch of a difference of O(1) terms (test_net_gpu.py)
        assert d["rel_l2"] <= NG.BF16_G0_TOL["rel_l2"] and d["cos"] >= NG.BF16_G0_TOL["cos"], (name, d)
    tol = NG.BF16_DP_TOL
    for name, d in cmp_p.items():
        assert d["rel_l2"] <= tol["rel_l2"] and d["cos"] >= tol["cos"] and abs(d["norm_ratio"] - 1) <= tol["norm"], (name, d)
    # the recorded distances to the clipped fixture (<= 2e-1) are not 10x the bf16 dP bar (8e-2): no separation is asserted here; the
    # fp32 replay and the kernel-level test make that point


# ---------------------------------------------------------------------------------------------- end to end
def _runner(task, num_envs, seed, monkeypatch):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    tc = task_registry.train_cfgs[args.task]
    tc.seed = seed
    monkeypatch.setattr(tc.algorithm, "use_clipped_value_loss", False)      # what train_cfg["algorithm"] sets
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


def test_runner_trains_unclipped_and_captured_update_equals_eager(monkeypatch, tmp_path):
    """XBot-L, 256 envs, bf16, algorithm.use_clipped_value_loss = False: three iterations with the update replayed from its HIP graph
    and three issued eagerly, same seeds: fused rollout, finite value loss, parameters / Adam moments / optimiser scalars
    bit-identical; a checkpoint round-trips."""
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "precision", "bf16")
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner("humanoid_ppo", 256, 78, monkeypatch)
        alg = r.alg
        assert alg.use_clipped_value_loss is False and alg._ppo_cfg.value_loss_unclipped == 1
        assert alg.net.shadow_ld(0) > 0 and r.env.rollout_fused_mode(alg.net) is not None
        r.env.episode_length_buf = torch.arange(256, device="cuda") * 7
        r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (mode == "1")
        opt = alg.net.opt_state.clone()
        assert int(opt[L.OPT_STEP]) == 3 * alg.num_learning_epochs * alg.num_mini_batches
        mean_value_loss = float(opt[L.OPT_VALUE_SUM]) / float(opt[L.OPT_MINIBATCHES])          # what the runner logs
        assert np.isfinite(mean_value_loss) and mean_value_loss > 0
        assert torch.isfinite(opt[:L.OPT_GRAD_SQNORM]).all() and torch.isfinite(alg.net.params).all()
        if mode == "1":
            # the captured update is keyed on the whole configuration: flipping the form asks for a new capture
            key = alg.update_graph_key()
            alg._ppo_cfg.value_loss_unclipped = 0
            assert alg.update_graph_key() != key
            alg._ppo_cfg.value_loss_unclipped = 1
            assert alg.update_graph_key() == key
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        outs[mode] = (alg.net.params.clone(), alg.net.adam_m.clone(), alg.net.adam_v.clone(), opt)
        if mode == "0":
            path = str(tmp_path / "model.pt")
            r.save(path)
            want = alg.net.params.clone()
            alg.net.params.add_(1.0)
            r.load(path)
            torch.cuda.synchronize()
            assert torch.equal(alg.net.params, want)
        del r
    for nm, a, b in zip(("params", "adam_m", "adam_v", "opt_state"), outs["1"], outs["0"]):
        assert torch.equal(a, b), nm


def test_dwl_runner_one_unclipped_iteration(monkeypatch):
    """humanoid_dwl_ppo (with the denoising head) under algorithm.use_clipped_value_loss = False: one iteration, finite."""
    torch.manual_seed(5)
    np.random.seed(5)
    r = _runner("humanoid_dwl_ppo", 256, 79, monkeypatch)
    alg = r.alg
    assert alg._ppo_cfg.value_loss_unclipped == 1 and alg._ppo_cfg.aux_coef > 0
    before = alg.net.params.clone()
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    opt = alg.net.opt_state
    assert np.isfinite(float(opt[L.OPT_VALUE_SUM]) / float(opt[L.OPT_MINIBATCHES])) and torch.isfinite(alg.net.params).all()
    assert not torch.equal(alg.net.params, before)
