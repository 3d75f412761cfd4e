"""-m gpu: the layer-by-layer path (csrc/hgym_net.hip GemmPath: gemm_nt_kernel, pack_rows_kernel, transpose_kernel, rowsum_kernel,
ppo_loss_kernel, reduce_slabs_kernel, adam_kernel) at 1 to 8 layers per net, ragged widths from 1 to 1000, num_actions 1 to 12 and batches
around every tile and padding boundary, against float64 references (tests/layer_path_common.py: the oracle's MLP with the case's activation;
for bf16 with the operands rounded where the kernels round them).  Which tile configurations and split counts the cases reach is pinned on
the CPU by tests/test_layer_path_shapes.py."""
import numpy as np
import pytest
import torch

import bf16_report as BR
import layer_path_common as LP
from oracle import ppo_oracle as P
from oracle import xbot_constants as K
from hgym import _lib as L

pytestmark = pytest.mark.gpu

FWD_TOL, FWD_MAX_TOL = 2e-3, 5e-3     # bf16 forward vs the bf16-operand reference: rel-L2 over the rows, worst output / output scale
F32_FWD_TOL = 1e-5                    # fp32 forward vs float64: worst output / output scale
GRAD_TOL = 5e-3                       # bf16 gradient vs the bf16-operand reference, per tensor rel-L2
F32_GRAD_TOL, F32_GRAD_TOL_BIG = 5e-5, 1e-4      # fp32 gradient per tensor; from B = 61 440 (accumulation order over the batch)
PRECISIONS = ["f32", "bf16"]


def _q64(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _random_mlp(dims, g):
    return P.Params.random(dims[0], dims[0], dims[-1], dims[1:-1], [], g).actor


def _setup(name, precision, max_batch, seed, lr=1e-3):
    """(actor, critic, aux layers (or None), std, NetBuffers) with random nn.Linear-style parameters loaded."""
    from hgym import NetBuffers
    no, npv, A, ah, ch, _, aux = LP.CASES[name]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    al = _random_mlp([no] + aux[0] + [aux[1]], g) if aux else None
    net = NetBuffers(LP.net_config(name, precision, max_batch), "cuda", learning_rate=lr)
    assert net.shadow_ld(0) == 0 and net.shadow_ld(1) == 0          # the layer-by-layer layout
    ts = list(p.tensors()) + ([t for W, b in al for t in (W, b)] if al else [])
    net.load_state_dict(dict(zip(list(net.views), ts)))
    return p, al, net, g


def _dbl(layers):
    return [(W.double(), b.double()) for W, b in layers]


def _split(net, flat):
    base = net.params.data_ptr()
    return [flat[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v) for v in net.views.values()]


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(LP.CASES))
def test_forward_at_every_batch_edge(name, precision):
    """hgym_mlp_forward of every net of the case at M in LP.FWD_M; a strided input (ldx > num_obs) gives the bits of its contiguous copy."""
    Mmax = max(LP.FWD_M)
    p, al, net, g = _setup(name, precision, Mmax, 21)
    no, npv, A, ah, ch, act, aux = LP.CASES[name]
    fwd, _ = LP.restated(act)
    q = _q64 if precision == "bf16" else None
    xs = {0: (torch.randn(Mmax, no, generator=g) * 2).clamp(-18, 18), 1: (torch.randn(Mmax, npv, generator=g) * 2).clamp(-18, 18)}
    nets = {0: p.actor, 1: p.critic}
    if al:
        xs[2], nets[2] = xs[0], al
    xd = {k: v.cuda() for k, v in xs.items()}
    for which, layers in nets.items():
        with torch.no_grad():
            ref = fwd(xs[which].double(), _dbl(layers), quant=q)
        scale = float(ref.abs().max())
        for m in LP.FWD_M:
            y = net.forward(which, xd[which][:m])
            torch.cuda.synchronize()
            d = y.cpu().double() - ref[:m]
            what = "layer path forward %s %s net %d, M = %d" % (name, precision, which, m)
            if precision == "bf16":
                BR.check(what + ", rel-L2", float(d.norm() / ref[:m].norm().clamp_min(1e-30)), FWD_TOL)
                BR.check(what + ", worst output", float(d.abs().max()) / scale, FWD_MAX_TOL)
            else:
                BR.check(what + ", worst output", float(d.abs().max()) / scale, F32_FWD_TOL)
        # strided rows: a column slice of a wider tensor
        wide = torch.randn(333, xs[which].shape[1] + 7, device="cuda")
        sl = wide[:, 3:3 + xs[which].shape[1]]
        assert sl.stride(0) > sl.shape[1]
        a, b = net.forward(which, sl), net.forward(which, sl.contiguous())
        torch.cuda.synchronize()
        assert torch.equal(a, b), (name, precision, which)


# ---------------------------------------------------------------------------------------------- gradient
def _storage(name, S, p, g):
    no, npv, A = LP.CASES[name][:3]
    obs, priv = torch.randn(S, no, generator=g), torch.randn(S, npv, generator=g)
    actions, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    fwd, _ = LP.restated(LP.CASES[name][5])
    with torch.no_grad():
        mu_now = fwd(obs, p.actor)
    lp_o = P.gaussian_log_prob(actions, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    return (obs, priv, actions, val, adv, ret, lp_o, mu_o, sg_o)


def _reference(name, precision, p, al, cols, idx, aux_coef, monkeypatch):
    """float64 gradient (flat list in state_dict order) and loss scalars of one minibatch."""
    act = LP.CASES[name][5]
    fwd, bwd = LP.restated(act)
    monkeypatch.setattr(P, "mlp_forward", fwd)
    monkeypatch.setattr(P, "mlp_backward", bwd)
    q = _q64 if precision == "bf16" else None
    pd = P.Params(_dbl(p.actor), _dbl(p.critic), p.std.double())
    rows = [t[idx].double() for t in cols]
    want = P.ppo_loss_and_grads(pd, *rows, quant=q)
    grads = list(want["grads"].tensors())
    if al:
        _, _, _, _, _, _, (hid, no_, off) = LP.CASES[name]
        B = idx.numel()
        y, acts, pres = fwd(rows[0], _dbl(al), keep=True, quant=q)
        dy = 2.0 * aux_coef * (y - rows[1][:, off:off + no_]) / (B * no_)
        for W, b in bwd(dy, _dbl(al), acts, pres, quant=q):
            grads += [W, b]
    return grads, want


def _check_grad(name, precision, B, net, grads_ref, want, opt0, what):
    got = [t.cpu() for t in _split(net, net.grads)]
    errs = {k: _rel_l2(a, r) for k, a, r in zip(net.views, got, grads_ref)}
    # the critic's head bias is ONE number, the sum of the B per-sample value-loss gradients, which cancel to a fraction of their size:
    # measured against the size of its terms, ||d_val||_2 (tests/test_activations_gpu.py)
    kb = [k for k in net.views if k.startswith("critic.")][-1]
    i = list(net.views).index(kb)
    errs[kb] = float((got[i].double() - grads_ref[i]).norm() / want["d_val"].double().norm())
    worst = max(errs, key=errs.get)
    bar = GRAD_TOL if precision == "bf16" else (F32_GRAD_TOL_BIG if B >= LP.BIG_B else F32_GRAD_TOL)
    BR.check("%s (worst tensor: %s)" % (what, worst), errs[worst], bar)
    opt = net.opt_state.cpu()
    rtol, atol = (1e-4, 1e-6) if precision == "f32" else (1e-2, 1e-4)
    np.testing.assert_allclose(float(opt[L.OPT_KL_LAST]), float(want["kl"]), rtol=rtol, atol=atol)
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM] - opt0[4]), float(want["value_loss"]), rtol=rtol, atol=atol)
    np.testing.assert_allclose(float(opt[L.OPT_SURROGATE_SUM] - opt0[3]), float(want["surrogate"]), rtol=rtol, atol=atol)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(LP.CASES))
def test_gradient_at_every_batch_edge(name, precision, monkeypatch):
    """hgym_ppo_grad through a permutation, B in LP.GRAD_B (and 61 440 on the two big cases), one NetBuffers for all of them: per tensor
    against the float64 reference, KL / value loss / surrogate as tests/test_net_gpu.py checks them."""
    from hgym import make_ppo_config, make_batch
    Bs = LP.GRAD_B + ([LP.BIG_B] if name in LP.BIG_CASES else [])
    S = max(Bs) + 1000
    p, al, net, g = _setup(name, precision, max(Bs), 22)
    cols = _storage(name, S, p, g)
    dev = [t.cuda().contiguous() for t in cols]
    aux_coef = 0.5 if al else 0.0
    ppo = make_ppo_config(aux_coef=aux_coef)
    for B in Bs:
        idx = torch.randperm(S, generator=g)[:B].contiguous()
        grads_ref, want = _reference(name, precision, p, al, cols, idx, aux_coef, monkeypatch)
        opt0 = net.opt_state.cpu()
        net.ppo_grad(ppo, make_batch(*dev, idx.cuda()))
        torch.cuda.synchronize()
        _check_grad(name, precision, B, net, grads_ref, want, opt0, "layer path gradient %s %s, B = %d" % (name, precision, B))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gradient_past_32_row_sum_chunks(precision, monkeypatch):
    """B = 140 000 (fp32) / 270 000 (bf16): more than 32 chunks of 4 096 / 8 192 rows, so every rowsum_kernel workgroup sums two of them
    (18 / 17 slabs per bias).  Against the float64 reference at the gradient bars, and the same bits on a second call."""
    from hgym import make_ppo_config, make_batch
    name, B = LP.HUGE_CASE, LP.HUGE_B[precision]
    S = B + 1000
    p, al, net, g = _setup(name, precision, B, 29)
    cols = _storage(name, S, p, g)
    dev = [t.cuda().contiguous() for t in cols]
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    grads_ref, want = _reference(name, precision, p, al, cols, idx, 0.0, monkeypatch)
    batch = make_batch(*dev, idx.cuda())
    ppo = make_ppo_config()
    opt0 = net.opt_state.cpu()
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    _check_grad(name, precision, B, net, grads_ref, want, opt0, "layer path gradient %s %s, B = %d" % (name, precision, B))
    first = net.grads_ext.clone()
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    assert torch.equal(first, net.grads_ext)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stale_workspace_gives_the_bits_of_a_fresh_one(precision):
    """A gradient at B = 4 097, then at B = 333 with another permutation, on one NetBuffers: the second result has the bits of the same
    call on a fresh NetBuffers (operand rows clamped at M, contraction padding [B, Bp) zeroed by the loss kernel and the transposes)."""
    from hgym import make_ppo_config, make_batch
    name = "deep"
    S = 5000
    p, al, net, g = _setup(name, precision, 4097, 23)
    _, _, fresh, _ = _setup(name, precision, 4097, 23)
    dev = [t.cuda().contiguous() for t in _storage(name, S, p, g)]
    i1 = torch.randperm(S, generator=g)[:4097].contiguous().cuda()
    i2 = torch.randperm(S, generator=g)[:333].contiguous().cuda()
    ppo = make_ppo_config()
    net.ppo_grad(ppo, make_batch(*dev, i1))
    net.ppo_grad(ppo, make_batch(*dev, i2))
    fresh.ppo_grad(ppo, make_batch(*dev, i2))
    torch.cuda.synchronize()
    for k, a, b in zip(net.views, _split(net, net.grads), _split(fresh, fresh.grads)):
        assert torch.equal(a, b), k
    assert torch.equal(net.grads_ext[-1:], fresh.grads_ext[-1:])      # the KL slot


class _Flat:
    def __init__(self, ts):
        self.ts = ts

    def tensors(self):
        return self.ts


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["deep", "with_aux"])
def test_apply_matches_clip_and_adam_and_keeps_the_operand_copies(name, precision):
    """hgym_ppo_apply twice on random gradients: the parameters move as the oracle's clip_grad_norm + Adam move them on the kernel's own
    gradient, and the workspace is byte-identical to a hgym_net_sync_shadow refresh from the master parameters (the ragged Wp / WTp images
    of every layer, tests/test_fused_gpu.py's check on the layer-by-layer layout)."""
    from hgym import make_ppo_config
    lr = 1e-3
    _, _, net, _ = _setup(name, precision, 512, 24, lr=lr)
    gd = torch.Generator(device="cuda").manual_seed(5)
    net.grads.copy_(torch.randn(net.P, device="cuda", generator=gd))
    torch.cuda.synchronize()
    p_ref = _Flat([t.cpu().clone() for t in _split(net, net.params)])
    p0 = [t.clone() for t in p_ref.tensors()]
    opt = P.Adam(p_ref)
    ppo = make_ppo_config(adaptive=False)
    for _ in range(2):
        g_ref = _Flat([t.cpu().clone() for t in _split(net, net.grads)])       # (adam_kernel leaves the clipped gradient in grads)
        P.clip_grad_norm(g_ref, 1.0)
        opt.step(p_ref, g_ref, lr)
        net.ppo_apply(ppo)
        torch.cuda.synchronize()
    got = [t.cpu() for t in _split(net, net.params)]
    d_got = torch.cat([(a - b).flatten() for a, b in zip(got, p0)])
    d_ref = torch.cat([(a - b).flatten() for a, b in zip(p_ref.tensors(), p0)])
    BR.check("layer path apply %s %s: parameter change vs clip_grad_norm + Adam, rel-L2" % (name, precision), _rel_l2(d_got, d_ref), 1e-5)
    after = net.workspace.clone()
    net.sync_shadow()
    torch.cuda.synchronize()
    assert torch.equal(after, net.workspace)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["thin", "pad", "wide"])
def test_policy_act_with_given_draws(name, precision):
    """hgym_policy_act with z supplied, num_actions 1 / 5 / 11: actions, sigma, logp and values against float64."""
    M = 333
    p, _, net, g = _setup(name, precision, M, 25)
    no, npv, A, _, _, act, _ = LP.CASES[name]
    fwd, _ = LP.restated(act)
    q = _q64 if precision == "bf16" else None
    obs, priv, z = torch.randn(M, no, generator=g), torch.randn(M, npv, generator=g), torch.randn(M, A, generator=g)
    with torch.no_grad():
        mu = fwd(obs.double(), _dbl(p.actor), quant=q)
        v = fwd(priv.double(), _dbl(p.critic), quant=q)
    sig = mu * 0 + p.std.double()
    a = mu + sig * z.double()
    lp = P.gaussian_log_prob(a, mu, sig)
    out = net.act(obs.cuda(), priv.cuda(), z=z.cuda())
    torch.cuda.synchronize()
    tol = FWD_MAX_TOL if precision == "bf16" else F32_FWD_TOL
    for key, ref in (("actions", a), ("mu", mu), ("values", v), ("logp", lp)):
        d = out[key].cpu().double().reshape(ref.shape) - ref
        BR.check("layer path act %s %s: %s, worst / scale" % (name, precision, key), float(d.abs().max() / ref.abs().max()), tol)
    assert torch.equal(out["sigma"].cpu(), (p.std * torch.ones(M, 1)).float())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("path", ["deep", "xbotl_no_fused"])
def test_gradient_at_the_baseline_minibatch_is_reproducible(path, precision, monkeypatch):
    """ppo_grad three times at B = 61 440 (15 / 8 row-sum chunks per bias in fp32 / bf16): the same bits every time -- on a layer-by-layer
    case and at the XBot-L widths with the fused kernels switched off."""
    from hgym import NetBuffers, make_net_config, make_ppo_config, make_batch
    B, S = LP.BIG_B, LP.BIG_B + 4096
    if path == "deep":
        p, _, net, g = _setup("deep", precision, B, 26)
        name = "deep"
    else:
        monkeypatch.setenv("HGYM_NO_FUSED", "1")
        g = torch.Generator().manual_seed(26)
        p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
        p.std = torch.rand(12, generator=g) * 0.5 + 0.75
        net = NetBuffers(make_net_config(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, precision, B), "cuda")
        assert net.shadow_ld(0) == 0
        net.load_state_dict(dict(zip(list(net.views), p.tensors())))
        name = None
    no, npv, A = (LP.CASES[name][:3] if name else (705, 219, 12))
    dev = "cuda"
    gd = torch.Generator(device=dev).manual_seed(27)
    cols = [torch.randn(S, no, device=dev, generator=gd), torch.randn(S, npv, device=dev, generator=gd),
            torch.randn(S, A, device=dev, generator=gd), torch.randn(S, device=dev, generator=gd), torch.randn(S, device=dev, generator=gd),
            torch.randn(S, device=dev, generator=gd), torch.randn(S, device=dev, generator=gd) - 5.0,
            torch.randn(S, A, device=dev, generator=gd) * 0.3, torch.rand(S, A, device=dev, generator=gd) * 0.5 + 0.75]
    idx = torch.randperm(S, device=dev, generator=gd)[:B].contiguous()
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config()
    runs = []
    for _ in range(3):
        net.ppo_grad(ppo, batch)
        runs.append(net.grads_ext.clone())
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0]).all()
    for r in runs[1:]:
        diff = [k for k, a, b in zip(net.views, _split(net, runs[0]), _split(net, r)) if not torch.equal(a, b)]
        assert not diff, "first differing tensor: %s" % diff[0]
        assert torch.equal(runs[0], r)


@pytest.mark.parametrize("max_batch", [40, 64, 100])
@pytest.mark.parametrize("path", ["pad-f32", "pad-bf16", "fused"])
def test_critic_values_walks_pieces_of_at_most_max_batch(path, max_batch):
    """hgym_critic_values over M in {1, 63, 65, 200} rows (M may exceed max_batch: include/hgym.h) on the layer-by-layer path and on the
    fused path, against the float64 critic."""
    from hgym import NetBuffers, make_net_config
    if path == "fused":
        g = torch.Generator().manual_seed(28)
        p = P.Params.random(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, g)
        net = NetBuffers(make_net_config(705, 219, 12, K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, "bf16", max_batch), "cuda")
        assert net.shadow_ld(1) > 0
        net.load_state_dict(dict(zip(list(net.views), p.tensors())))
        fwd, npv, precision = P.mlp_forward, 219, "bf16"
    else:
        precision = path.split("-")[1]
        p, _, net, g = _setup("pad", precision, max_batch, 28)
        fwd, _ = LP.restated(LP.CASES["pad"][5])
        npv = LP.CASES["pad"][1]
    priv = (torch.randn(200, npv, generator=g) * 2).clamp(-18, 18)
    with torch.no_grad():
        ref = fwd(priv.double(), _dbl(p.critic), quant=_q64 if precision == "bf16" else None).squeeze(1)
    scale = float(ref.abs().max())
    pd = priv.cuda()
    for M in (1, 63, 65, 200):
        vals = torch.full((M,), float("nan"), device="cuda")
        net.critic_values(pd[:M].contiguous(), vals)
        torch.cuda.synchronize()
        d = vals.cpu().double() - ref[:M]
        what = "critic_values %s max_batch %d, M = %d" % (path, max_batch, M)
        if precision == "bf16":
            BR.check(what + ", rel-L2", float(d.norm() / ref[:M].norm()), FWD_TOL)
            BR.check(what + ", worst output", float(d.abs().max()) / scale, FWD_MAX_TOL)
        else:
            BR.check(what + ", worst output", float(d.abs().max()) / scale, F32_FWD_TOL)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("precision", PRECISIONS)
def test_runner_trains_the_deep_case_and_captured_update_equals_eager(precision, monkeypatch):
    """make_alg_runner / learn with the `deep` hidden widths (8 + 8 layers), 1 024 envs (60 steps: minibatches of 15 360 rows, four / two
    row-sum chunks in fp32 / bf16): two iterations with the update replayed from its HIP graph and two issued eagerly (HGYM_GRAPH_UPDATE=0), same seeds --
    parameters, Adam moments and optimiser scalars bit-identical (tests/test_fused_shapes_gpu.py's check at other widths)."""
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    monkeypatch.setattr(PPO, "precision", precision)
    ah, ch = LP.CASES["deep"][3], LP.CASES["deep"][4]
    N = 1024
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N), "--seed", "78"])
        tc = task_registry.train_cfgs[args.task]
        tc.seed = 78
        monkeypatch.setattr(tc.policy, "actor_hidden_dims", list(ah))
        monkeypatch.setattr(tc.policy, "critic_hidden_dims", list(ch))
        env, _ = task_registry.make_env(name=args.task, args=args)
        r, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
        alg = r.alg
        assert alg.net.cfg.actor_layers == 8 and alg.net.cfg.critic_layers == 8 and alg.net.shadow_ld(0) == 0
        r.env.episode_length_buf = torch.arange(N, device="cuda") * 7
        r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
        torch.cuda.synchronize()
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
