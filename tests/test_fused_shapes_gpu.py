"""-m gpu: the fused bf16 MLP kernels (csrc/hgym_fused.hpp: mlp_fwd_kernel, mlp_fb_kernel, dw_kernel_rs, adam_kernel's fragment
writes) at network widths other than XBot-L's, chosen so that every instantiation and branch of the family fused_supported() accepts
runs: fwd_body / fb_body at all three first widths, the `pre` gather of the loss inputs switched off (third width > 128, or
num_actions != 12), a second width larger than the first, and shapes whose update tile does not fit in LDS, which must take the
generic bf16 path from creation on (tests/test_fused_shapes.py pins that decision over the whole family on the host).

References: oracle/ppo_oracle.py evaluated in float64 on bf16-rounded operands (quant = bf16 rounding where the kernels round), and
the oracle's clip_grad_norm + Adam on the kernel's own gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_report as BR
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu

BF16_OPERAND_TOL = 5e-3      # fused kernels vs the bf16-operand oracle, per tensor, rel-L2 (tests/test_fused_gpu.py)
# forward vs the bf16-operand oracle: rel-L2 over all M rows <= 2e-3 (the bar tests/test_fused_gpu.py puts on the fused forward), and the
# worst single output <= 5e-3 of the output scale.  The worst output grows with M: where the kernel's fp32 sums and the oracle's float64
# ones fall on two sides of a bf16 rounding boundary, a hidden activation differs by one bf16 step -- measured worst 1.8e-3 at 5000 rows
# (narrow actor), 2.3e-3 at 20000 (wide3 actor, 188 / 146 inputs); rel-L2 at most 4.5e-4.  A row the kernel got wrong would be off by the
# output scale itself.
FWD_TOL = 2e-3
FWD_MAX_TOL = 5e-3

# name: (actor hidden, critic hidden, num_actions, fused) -- what the row reaches, mlp_fb_kernel LDS actor / critic from the formulas
ROWS = {
    "xbotl": ([512, 256, 128], [768, 256, 128], 12, True),         # control: 133 504 / 157 568 B
    "g1": ([256, 256, 256], [256, 256, 256], 12, True),            # fb_body<1> / fwd_body<U> on both nets, `pre` off: 116 608 / 106 880
    "narrow": ([256, 128, 128], [768, 128, 128], 12, True),        # narrowest trunk: 99 200 / 157 056
    "wide3": ([512, 256, 256], [512, 256, 384], 12, True),         # third width > 128 (`pre` off) on both nets: 150 400 / 157 568
    "n1gtn0": ([256, 640, 128], [256, 768, 128], 12, True),        # second width > first (H1 / dZ1 sized by Q): 150 400 / 157 568
    "a10": ([512, 384, 128], [512, 512, 128], 10, True),           # A != 12: the scalar loss / head branches: 150 400 / 157 568
    "big_actor": ([768, 256, 128], [768, 256, 128], 12, False),    # 167 296 B > 160 KiB: generic bf16 path
    "large": ([768, 768, 768], [768, 768, 768], 12, False),        # 319 360 / 309 632 B: generic path, large widths
}
# XBot-L's input widths everywhere, and a ragged pair (4 x 47 / 2 x 73) on two rows
CASES = [(r, 705, 219) for r in ROWS] + [("g1", 188, 146), ("wide3", 188, 146)]
IDS = ["%s-%d-%d" % c for c in CASES]
# the generic bf16 path (the two refused rows) against the same bf16-operand oracle, the same bar: measured worst tensor 2.4e-3
GENERIC_GRAD_TOL = 5e-3
# hgym_ppo_apply vs the oracle's clip + Adam on the same gradient, fp32 on both sides: max |parameter difference| / learning rate.
# Measured at most 1.5e-5 on every row: two fp32 steps of a parameter of ~0.06 (the step size is a float in the kernel, a double in the oracle).
APPLY_TOL = 5e-5


def _dbl(layers):
    return [(W.double(), b.double()) for W, b in layers]


def _q64(t):
    """bf16 round-to-nearest-even, kept in the tensor's own precision (the float64 oracle)."""
    return t.to(torch.bfloat16).to(t.dtype)


def _setup(row, n_obs, n_priv, max_batch, seed):
    from hgym import NetBuffers, make_net_config
    ah, ch, A, _ = ROWS[row]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(n_obs, n_priv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    net = NetBuffers(make_net_config(n_obs, n_priv, A, ah, ch, "bf16", max_batch), "cuda", learning_rate=1e-3)
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    return p, net, g


def _rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _split(net, flat):
    """Per-tensor views of a flat (P,) vector, in state_dict order."""
    base = net.params.data_ptr()
    return [flat[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v) for v in net.views.values()]


@pytest.mark.parametrize("row,n_obs,n_priv", CASES, ids=IDS)
def test_path_follows_the_lds_budget(row, n_obs, n_priv):
    _, net, _ = _setup(row, n_obs, n_priv, 64, 0)
    want = ((n_obs + 127) // 128 * 128, (n_priv + 127) // 128 * 128) if ROWS[row][3] else (0, 0)
    assert (net.shadow_ld(0), net.shadow_ld(1)) == want


@pytest.mark.parametrize("row,n_obs,n_priv", CASES, ids=IDS)
def test_forward_vs_bf16_operand_oracle(row, n_obs, n_priv):
    """M = 1, 100, 5000 (32-row tiles) and 20000 (64-row tiles) rows through hgym_mlp_forward, actor and critic, against the
    float64 oracle on bf16 operands (bounds at FWD_TOL)."""
    Mmax = 20000
    p, net, g = _setup(row, n_obs, n_priv, Mmax, 1)
    obs = (torch.randn(Mmax, n_obs, generator=g) * 2).clamp(-18, 18)
    priv = (torch.randn(Mmax, n_priv, generator=g) * 2).clamp(-18, 18)
    with torch.no_grad():
        ref = {0: P.mlp_forward(obs.double(), _dbl(p.actor), quant=_q64), 1: P.mlp_forward(priv.double(), _dbl(p.critic), quant=_q64)}
    xs = {0: obs.cuda(), 1: priv.cuda()}
    for M in (1, 100, 5000, Mmax):
        for which in (0, 1):
            y = net.forward(which, xs[which][:M].contiguous())
            torch.cuda.synchronize()
            d, r = y.cpu().double() - ref[which][:M], ref[which][:M]
            what = "forward %s %s, %d / %d inputs, M = %d vs bf16-operand oracle" % (row, ("actor", "critic")[which], n_obs, n_priv, M)
            BR.check(what + ", rel-L2", float(d.norm() / r.norm()), FWD_TOL)
            BR.check(what + ", worst output", float(d.abs().max() / ref[which].abs().max()), FWD_MAX_TOL)


def _grad_inputs(p, n_obs, n_priv, A, S, g):
    obs, priv = torch.randn(S, n_obs, generator=g), torch.randn(S, n_priv, generator=g)
    act, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = P.mlp_forward(obs, p.actor)
    # old log-probs near the current policy's: ratios on both sides of the clip range
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    return obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o


def _oracle_grad(p, cols, idx):
    obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o = (t[idx].double() for t in cols)
    pd = P.Params(_dbl(p.actor), _dbl(p.critic), p.std.double())
    return P.ppo_loss_and_grads(pd, obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o, quant=_q64)


@pytest.mark.parametrize("S,B", [(700, 333), (5000, 4096)])
@pytest.mark.parametrize("row,n_obs,n_priv", CASES, ids=IDS)
def test_gradient_apply_and_shadows(row, n_obs, n_priv, S, B):
    """(1) hgym_ppo_grad twice on the same minibatch (the second call must not depend on what the first left) against the float64
    bf16-operand oracle, per parameter tensor in rel-L2, and the loss scalars.  (2) hgym_ppo_apply on the kernel's own gradient, scaled
    to a norm above max_grad_norm (clip active) and then below it, against the oracle's clip_grad_norm + Adam.step on the same
    gradient.  (3) After the two steps the bf16 operand copies adam_kernel wrote equal, byte for byte, what hgym_net_sync_shadow
    re-derives from the masters."""
    from hgym import make_ppo_config, make_batch
    _, _, A, fused = ROWS[row]
    p, net, g = _setup(row, n_obs, n_priv, max(B, 512), S + B)
    cols = _grad_inputs(p, n_obs, n_priv, A, S, g)
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    want = _oracle_grad(p, cols, idx)
    keep = [t.cuda().contiguous() for t in cols] + [idx.cuda()]
    for _ in range(2):
        net.ppo_grad(make_ppo_config(), make_batch(*keep))
    torch.cuda.synchronize()
    tol = BF16_OPERAND_TOL if fused else GENERIC_GRAD_TOL
    errs = {k: _rel_l2(got.cpu(), r) for k, got, r in zip(net.views, _split(net, net.grads), want["grads"].tensors())}
    BR.check("%s gradient %s, %d / %d inputs, S = %d, B = %d vs bf16-operand oracle (worst tensor)" % (
        "fused" if fused else "generic", row, n_obs, n_priv, S, B), max(errs.values()), tol)
    opt = net.opt_state.cpu()
    np.testing.assert_allclose(float(opt[L.OPT_KL_LAST]), float(want["kl"]), rtol=2e-2, atol=1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM]) / 2, float(want["value_loss"]), rtol=1e-2)

    # (2) Adam on a known gradient
    g0 = net.grads.clone()
    assert float(net.opt_state[L.OPT_STEP]) == 0.0
    ppo = make_ppo_config(max_grad_norm=1.0, adaptive=False)
    lr = float(net.opt_state[L.OPT_LR])
    ref_p = P.Params([(W.clone(), b.clone()) for W, b in p.actor], [(W.clone(), b.clone()) for W, b in p.critic], p.std.clone())
    adam = P.Adam(ref_p)
    for step, norm in enumerate((3.0, 0.5)):
        gk = g0 * (norm / float(g0.double().norm()))
        net.grads.copy_(gk)
        net.ppo_apply(ppo)
        torch.cuda.synchronize()
        gs = [t.cpu().clone() for t in _split(net, gk)]
        rg = P.Params([(gs[1 + 2 * i], gs[2 + 2 * i]) for i in range(4)], [(gs[9 + 2 * i], gs[10 + 2 * i]) for i in range(4)], gs[0])
        total = float(P.clip_grad_norm(rg, 1.0))
        adam.step(ref_p, rg, lr)
        assert float(net.opt_state[L.OPT_STEP]) == step + 1 and float(net.opt_state[L.OPT_LR]) == lr
        np.testing.assert_allclose(float(net.opt_state[L.OPT_GRAD_NORM]), total, rtol=1e-5)
        err = max(float((v.cpu() - r).abs().max()) for v, r in zip(net.views.values(), ref_p.tensors())) / lr
        BR.check("apply (fp32) %s, S = %d, B = %d, step %d (gradient norm %.1f): max |param - oracle| / lr" % (row, S, B, step, norm),
                 err, APPLY_TOL)

    # (3) operand copies
    after_adam = net.workspace.clone()
    net.sync_shadow()
    torch.cuda.synchronize()
    assert torch.equal(after_adam, net.workspace)


@pytest.mark.parametrize("row,n_obs,n_priv", [("g1", 705, 219), ("wide3", 705, 219), ("g1", 188, 146)], ids=["g1", "wide3", "g1-ragged"])
@pytest.mark.parametrize("S,B", [(700, 333), (5000, 4096)])
def test_update_from_the_bf16_shadow_equals_update_from_fp32_rows(row, n_obs, n_priv, S, B):
    """mlp_fb_kernel<true> (first layer gathered from the bf16 input shadow) against mlp_fb_kernel<false> on the fp32 rows, on the
    G1 = 1 and the `pre`-off shapes: the gradients and loss sums are bit-identical."""
    from hgym import make_ppo_config, make_batch
    _, _, A, _ = ROWS[row]
    p, net, g = _setup(row, n_obs, n_priv, max(B, 512), 3 * S + B)
    cols = [t.cuda().contiguous() for t in _grad_inputs(p, n_obs, n_priv, A, S, g)]
    idx = torch.randperm(S, generator=g)[:B].contiguous().cuda()
    lo, lp = net.shadow_ld(0), net.shadow_ld(1)
    assert lo > 0 and lp > 0
    so = torch.zeros(S, lo, dtype=torch.bfloat16, device="cuda")
    sp = torch.zeros(S, lp, dtype=torch.bfloat16, device="cuda")
    so[:, :n_obs] = cols[0].to(torch.bfloat16)
    sp[:, :n_priv] = cols[1].to(torch.bfloat16)
    net.ppo_grad(make_ppo_config(), make_batch(*cols, idx))
    torch.cuda.synchronize()
    want, want_opt = net.grads_ext.clone(), net.opt_state.clone()
    net.grads_ext.zero_()
    net.opt_state[L.OPT_KL_SUM:L.OPT_GRAD_SQNORM + 1] = 0.0
    net.ppo_grad(make_ppo_config(), make_batch(*cols, idx, obs_bf16=so, priv_bf16=sp))
    torch.cuda.synchronize()
    assert torch.equal(net.grads_ext, want)
    assert torch.equal(net.opt_state[L.OPT_KL_SUM:L.OPT_GRAD_SQNORM], want_opt[2:9])
    np.testing.assert_allclose(float(net.opt_state[L.OPT_GRAD_SQNORM]), float(want_opt[9]), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ auxiliary (denoising) head
AUX_CASES = {"fused": ([512, 256, 256], 73, True),      # mlp_fb_kernel LDS 148 608 B: the head's own fused launches
             "refused": ([512, 768, 128], 96, False)}   # 199 360 B: the head alone takes the generic path
AUX_GENERIC_TOL = 5e-3      # the generic head against the same oracle, the same bar: measured worst tensor 1.0e-3


@pytest.mark.parametrize("case", list(AUX_CASES))
def test_aux_head_gradient_vs_oracle(case, monkeypatch):
    """XBot-L trunk + a denoiser head regressing the last `out` columns of the privileged row (coef * MSE): the head's gradient against
    the float64 bf16-operand oracle (mlp_backward of dL/dy = 2 coef (y - t) / (B out)), the trunk's against ppo_loss_and_grads, the
    head's loss in opt_state[10].  Whether the head kept its fused layout is read off the workspace size (HGYM_NO_FUSED_AUX)."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch, _lib as L
    hidden, out, fused = AUX_CASES[case]
    S, B, coef = 900, 700, 0.5
    off = 219 - out
    cfg = make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], "bf16", B, aux_hidden=hidden, aux_out=out, aux_target_offset=off)
    ws = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
    monkeypatch.setenv("HGYM_NO_FUSED_AUX", "1")
    ws_generic = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
    monkeypatch.delenv("HGYM_NO_FUSED_AUX")
    assert (ws != ws_generic) == fused
    net = NetBuffers(cfg, "cuda", learning_rate=1e-3)
    assert net.shadow_ld(0) == 768
    g = torch.Generator().manual_seed(17)
    p = P.Params.random(705, 219, 12, [512, 256, 128], [768, 256, 128], g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    head = P.Params.random(705, 219, out, hidden, [8, 8, 8], g).actor
    trunk = [k for k in net.views if not k.startswith("denoiser")]
    sd = dict(zip(trunk, p.tensors()))
    for l, (W, b) in enumerate(head):
        sd["denoiser.%d.weight" % (2 * l)], sd["denoiser.%d.bias" % (2 * l)] = W, b
    net.load_state_dict(sd)
    cols = _grad_inputs(p, 705, 219, 12, S, g)
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    want = _oracle_grad(p, cols, idx)
    x, t = cols[0][idx].double(), cols[1][idx].double()[:, off:off + out]
    hd = _dbl(head)
    with torch.no_grad():
        y, acts, pres = P.mlp_forward(x, hd, keep=True, quant=_q64)
        mse = float(((y - t) ** 2).mean())
        hg = P.mlp_backward(2.0 * coef * (y - t) / (B * out), hd, acts, pres, quant=_q64)
    keep = [c.cuda().contiguous() for c in cols] + [idx.cuda()]
    for _ in range(2):                  # twice: nothing may carry over from the first call
        net.opt_state[L.OPT_AUX_SUM] = 0.0
        net.ppo_grad(make_ppo_config(aux_coef=coef), make_batch(*keep))
    torch.cuda.synchronize()
    gv = net.grad_views()
    for k, r in zip(trunk, want["grads"].tensors()):
        assert _rel_l2(gv[k].cpu(), r) <= BF16_OPERAND_TOL, (k, _rel_l2(gv[k].cpu(), r))
    tol = BF16_OPERAND_TOL if fused else AUX_GENERIC_TOL
    errs = {}
    for l, (gw, gb) in enumerate(hg):
        for nm, r in (("weight", gw), ("bias", gb)):
            errs[(l, nm)] = _rel_l2(gv["denoiser.%d.%s" % (2 * l, nm)].cpu(), r)
    BR.check("denoiser %s -> %d (%s) gradient vs bf16-operand oracle (worst tensor)" % (hidden, out, case), max(errs.values()), tol)
    np.testing.assert_allclose(float(net.opt_state[L.OPT_AUX_SUM]), mse, rtol=1e-2)


# ------------------------------------------------------------------------------------------------ end to end
def _runner(num_envs, seed, actor_hidden, critic_hidden, monkeypatch):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    tc = task_registry.train_cfgs[args.task]
    tc.seed = seed
    monkeypatch.setattr(tc.policy, "actor_hidden_dims", list(actor_hidden))
    monkeypatch.setattr(tc.policy, "critic_hidden_dims", list(critic_hidden))
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


@pytest.mark.parametrize("actor_hidden,critic_hidden,fused", [([256, 256, 256], [256, 256, 256], True),
                                                              ([768, 256, 128], [768, 256, 128], False),
                                                              ([512, 256, 128], [768, 256, 256], False)],
                         ids=["256-256-256", "768-256-128", "xbotl-actor-critic-768-256-256"])
def test_runner_trains_at_other_widths_and_captured_update_equals_eager(actor_hidden, critic_hidden, fused, monkeypatch):
    """make_alg_runner / learn, 256 envs, bf16, at the given widths: two iterations with the update replayed from its HIP graph and two
    with it issued eagerly (HGYM_GRAPH_UPDATE=0), same seeds: finite losses, Adam's step count, and parameters, Adam moments and
    optimiser scalars bit-identical.  None of these takes the fused rollout step (hgym_rollout_step): it serves first widths 512 / 768
    only, and only on a fused net -- the last case has XBot-L's first widths, but its critic's update tile (174 464 B) does not fit, so the
    net runs the generic path and the runner must pick PPO.act + the env step for it."""
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "precision", "bf16")
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(256, 78, actor_hidden, critic_hidden, monkeypatch)
        alg = r.alg
        assert list(alg.net.cfg.actor_dims)[1:4] == list(actor_hidden) and list(alg.net.cfg.critic_dims)[1:4] == list(critic_hidden)
        assert (alg.net.shadow_ld(0) > 0) == fused
        assert r.env.rollout_fused_mode(alg.net) is None
        r.env.episode_length_buf = torch.arange(256, device="cuda") * 7
        r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        assert (alg.storage._obs_bf16 is not None) == fused
        assert (r._update_graph is not None) == (mode == "1")
        assert int(alg.net.opt_state[L.OPT_STEP]) == 2 * alg.num_learning_epochs * alg.num_mini_batches
        opt = alg.net.opt_state.clone()
        assert torch.isfinite(opt[:L.OPT_GRAD_SQNORM]).all() and torch.isfinite(alg.net.params).all()
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        outs[mode] = (alg.net.params.clone(), alg.net.adam_m.clone(), alg.net.adam_v.clone(), opt)
        del r
    for nm, a, b in zip(("params", "adam_m", "adam_v", "opt_state"), outs["1"], outs["0"]):
        assert torch.equal(a, b), nm
