"""-m gpu: empirical observation normalisation at the library level (csrc/hgym_norm.hip and the first-layer fold in csrc/hgym_net.hip; DESIGN.md
section 22), through hgym.NetBuffers.

1. accumulate + merge against float64 (tests/obs_norm_common.py), at the bounds derived there;
2. the fold on the fp32 layer-by-layer path, ragged small net: a normalised net on raw rows against a plain net on explicitly normalised rows
   and against float64 autograd, at tests/test_net_gpu.py's fp32 bars;
3. the fold on the fused bf16 path at XBot-L's widths: power-of-two scales make the two nets agree BIT FOR BIT; a general state is held
   against the float64 bf16-operand oracle (tests/fused_batch_common.py) fed the folded parameters;
4. off is off: a block at its initial state with eps = 0 (scale exactly 1, mean 0) changes no bit of two optimiser steps."""
import numpy as np
import pytest
import torch

import fused_batch_common as FB
import obs_norm_common as ON
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu
F32_FWD_BAR, F32_GRAD_BAR = 1e-5, 5e-5      # tests/test_net_gpu.py: max-abs error over max-abs reference


def _net(no, npv, A, ah, ch, precision, max_batch, obs_norm=None, lr=1e-3, aux=None):
    """aux: (hidden widths, outputs, target offset) of an auxiliary head, or None."""
    from hgym import NetBuffers, make_net_config
    kw = {} if aux is None else dict(aux_hidden=aux[0], aux_out=aux[1], aux_target_offset=aux[2])
    return NetBuffers(make_net_config(no, npv, A, ah, ch, precision, max_batch, **kw), "cuda", learning_rate=lr, obs_norm=obs_norm)


def _names(n_layers_a, n_layers_c):
    return ["std"] + ["%s.%d.%s" % (n, 2 * l, k) for n, L_ in (("actor", n_layers_a), ("critic", n_layers_c)) for l in range(L_)
                      for k in ("weight", "bias")]


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(net):
    """(mean, var) of both statistics as float64 numpy, and the two counts."""
    h = net.norm_view("header").cpu().numpy()
    return [(net.norm_view("mean", k).cpu().numpy(), net.norm_view("var", k).cpu().numpy(), float(h[2 + k])) for k in (0, 1)]


# ------------------------------------------------------------------------------------------------ 1. accumulate + merge
def _columns(M, K, rng):
    """(M, K) fp32: columns offset by up to +-18, spread between 0.01 and 3; column 1 constant (7.3), column 2 all zero (where they exist)."""
    off = np.linspace(-18.0, 18.0, K) if K > 1 else np.array([18.0])
    spread = np.geomspace(0.01, 3.0, K)
    x = (off[None, :] + spread[None, :] * rng.standard_normal((M, K))).astype(np.float32)
    if K > 1:
        x[:, 1] = np.float32(7.3)
    if K > 2:
        x[:, 2] = 0.0
    return x


def _grid_pass(K0, K1):
    """The smallest row count beyond one pass of the accumulate launch's grid for both row kinds (+ a ragged tail)."""
    from hgym import make_net_config, norm_layout
    lay = norm_layout(make_net_config(K0, K1, 2, [8], [8], "f32", 64))
    return max(lay[L.NORM_WGS], lay[L.NORM_WGS + 1]) * lay[L.NORM_ROWS_PER_WG] + lay[L.NORM_ROWS_PER_WG] + 1


ROWS = 64       # hgym_net_norm_layout()[HGYM_NORM_ROWS_PER_WG], asserted below
SMALL_M = [1, 2, 3, 4, 5, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 3]
ACC_CASES = [(K, M) for K in ((705, 219), (219, 705), (3, 1), (1, 3)) for M in SMALL_M] + [((705, 219), "pass"), ((3, 1), "pass")]


@pytest.mark.parametrize("K,M", ACC_CASES)
def test_accumulate_and_merge_against_float64(K, M):
    """Three successive batches (M rows, then 7, then M + 3) merged on the device against the float64 merge of the same rows: count exact,
    |d mean| and |d var| within the per-merge bounds of obs_norm_common (added up over the merges so far: both chains carry their own
    state), the floats the kernels read re-derived from the device's own state within one fp32 ulp, the constant column's variance 0
    within the bound and its scale between 1 / (sqrt(bound) + eps) and 1 / eps, the zero column exact."""
    eps = 1e-2
    net = _net(K[0], K[1], 2, [8], [8], "f32", 64, obs_norm=(eps, None))
    assert net.norm_layout[L.NORM_ROWS_PER_WG] == ROWS
    M = _grid_pass(*K) if M == "pass" else M
    rng = np.random.default_rng(1000 * K[0] + (M % 997))
    ref = [ON.initial(K[0]), ON.initial(K[1])]
    bm, bv = [0.0, 0.0], [0.0, 0.0]
    for rows in (M, 7, M + 3):
        xs = [_columns(rows, K[k], rng) for k in (0, 1)]
        net.norm_accumulate(torch.from_numpy(xs[0]).cuda(), torch.from_numpy(xs[1]).cuda())
        sums = net.norm_view("sums").cpu().numpy()
        assert sums[0] == rows and sums[1 + 2 * K[0]] == rows
        net.norm_merge()
        torch.cuda.synchronize()
        got = _state(net)
        for k in (0, 1):
            ref[k] = ON.merge(ref[k], xs[k])
            dm, dv = ON.bounds(xs[k])
            bm[k] += dm
            bv[k] += dv
            mean, var, count = got[k]
            assert count == ref[k]["count"]
            assert np.isfinite(mean).all() and np.isfinite(var).all() and (var >= 0).all()
            em, ev = np.abs(mean - ref[k]["mean"]).max(), np.abs(var - ref[k]["var"]).max()
            print("K=%d rows=%d: |d mean| %.3e (bound %.3e)  |d var| %.3e (bound %.3e)" % (K[k], rows, em, bm[k], ev, bv[k]))
            assert em <= bm[k] and ev <= bv[k]
            mf, sf = net.norm_view("mean_f", k).cpu().numpy(), net.norm_view("scale_f", k).cpu().numpy()
            wm, ws = ON.derived(mean, var, eps)
            assert np.array_equal(mf, wm) and (np.abs(sf.astype(np.float64) - ws) <= 2.0 ** -23 * np.abs(ws)).all()
            if K[k] > 1:      # the constant column
                e = float(np.float32(eps))
                assert var[1] <= bv[k] and 1.0 / (np.sqrt(bv[k]) + e) * (1 - 2.0 ** -23) <= sf[1] <= np.float32(1.0 / e)
            if K[k] > 2:      # the all-zero column: every step exact
                assert mean[2] == 0.0 and var[2] == 0.0 and sf[2] == np.float32(1.0 / float(np.float32(eps))) and mf[2] == 0.0


def test_accumulate_is_reproducible_unaligned_rows_and_until():
    """The same rows give the same bits in a second run (fixed summation order, no atomics); rows that start 4 bytes off a 16-byte boundary
    take the 4-byte path and stay within the bounds; `until` stops the merges on the device once the count has reached it."""
    K, M = (705, 219), 2 * ROWS + 3
    rng = np.random.default_rng(7)
    xs = [_columns(M, K[k], rng) for k in (0, 1)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    runs = []
    for _ in range(2):
        net = _net(K[0], K[1], 2, [8], [8], "f32", 64, obs_norm=(1e-2, None))
        for _ in range(2):
            net.norm_accumulate(*dev)
            net.norm_merge()
        torch.cuda.synchronize()
        runs.append([net.norm_view(n, k).clone() for k in (0, 1) for n in ("mean", "var", "mean_f", "scale_f")] + [net.norm_view("sums").clone()])
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    # 4 bytes off: one float of padding in front of the rows
    net = _net(K[0], K[1], 2, [8], [8], "f32", 64, obs_norm=(1e-2, None))
    shifted = []
    for x in dev:
        buf = torch.zeros(x.numel() + 5, device="cuda")
        buf[1:1 + x.numel()] = x.flatten()
        shifted.append(buf[1:1 + x.numel()].view_as(x))
        assert shifted[-1].data_ptr() % 16 == 4 and shifted[-1].is_contiguous()
    net.norm_accumulate(*shifted)
    net.norm_merge()
    torch.cuda.synchronize()
    for k, (mean, var, count) in enumerate(_state(net)):
        ref = ON.merge(ON.initial(K[k]), xs[k])
        dm, dv = ON.bounds(xs[k])
        assert count == M and np.abs(mean - ref["mean"]).max() <= dm and np.abs(var - ref["var"]).max() <= dv
    # until = 100 rows: batches of 64 merge while count < 100 -- twice -- and never again
    net = _net(K[0], K[1], 2, [8], [8], "f32", 64, obs_norm=(1e-2, 100))
    counts, keep = [], None
    for i in range(4):
        net.norm_accumulate(dev[0][:64].contiguous(), dev[1][:64].contiguous())
        net.norm_merge()
        counts.append([c for _, _, c in _state(net)])
        if i == 1:
            keep = [net.norm_view(n, k).clone() for k in (0, 1) for n in ("mean", "var", "mean_f", "scale_f")]
    assert counts == [[64.0, 64.0], [128.0, 128.0], [128.0, 128.0], [128.0, 128.0]]
    assert all(_same_bits(a, b) for a, b in zip(keep, [net.norm_view(n, k) for k in (0, 1) for n in ("mean", "var", "mean_f", "scale_f")]))


# ------------------------------------------------------------------------------------------------ shared: planted statistics, rows, columns
def _plant(net, means, variances, count=1000.0):
    net.load_norm_state(dict(obs=dict(mean=torch.from_numpy(means[0]), var=torch.from_numpy(variances[0]), count=count),
                             critic_obs=dict(mean=torch.from_numpy(means[1]), var=torch.from_numpy(variances[1]), count=count)))
    torch.cuda.synchronize()
    return [(net.norm_view("mean_f", k).cpu().numpy(), net.norm_view("scale_f", k).cpu().numpy()) for k in (0, 1)]


def _planted_general(K, eps, g):
    """Per statistic: variances in [0.25, 4] with ONE var = 0 column, means with |m| s up to 3 (s = 1 / (sqrt(var) + eps))."""
    means, variances = [], []
    for k in K:
        var = (0.25 * 16.0 ** torch.rand(k, generator=g, dtype=torch.float64)).numpy()
        var[k // 2] = 0.0
        s = 1.0 / (np.sqrt(var) + float(np.float32(eps)))
        u = (torch.rand(k, generator=g, dtype=torch.float64) * 2 - 1).numpy()
        u[0], u[-1] = 1.0, -1.0
        means.append(3.0 * u / s)
        variances.append(var)
    return means, variances


def _raw_rows(S, mean, var, eps, g):
    """Rows whose normalised form is O(1): m + (sqrt(var) + eps) z."""
    z = torch.randn(S, mean.shape[0], generator=g, dtype=torch.float64).numpy()
    return (mean[None, :] + (np.sqrt(var) + eps)[None, :] * z).astype(np.float32)


def _columns_for(p, obs_n, priv_n, A, g, quant=None):
    """The seven other batch columns for rows whose NORMALISED form is obs_n / priv_n (what the master parameters p see): old
    log-probabilities near the current policy's, so that ratios fall on both sides of the clip range (fused_batch_common.grad_inputs)."""
    S = obs_n.shape[0]
    act, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = P.mlp_forward(obs_n.double(), FB.dbl(p.actor), quant=quant)
    lp_o = (P.gaussian_log_prob(act.double(), mu_now, mu_now * 0 + p.std.double()) + torch.randn(S, generator=g).double() * 0.3).float()
    return [act, val, adv, ret, lp_o, mu_o, sg_o]


def _grad(net, obs, priv, rest, idx, unfold, aux_coef=0.0):
    from hgym import make_batch, make_ppo_config
    ppo = make_ppo_config(grad_norm_ready=False, aux_coef=aux_coef)
    cols = [t.cuda().contiguous() for t in [obs, priv] + rest]
    net.ppo_grad(ppo, make_batch(*cols, idx.cuda()))
    if unfold:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    return ppo, cols


# ------------------------------------------------------------------------------------------------ 2. fold, fp32 path
def test_fold_f32_ragged_net_against_plain_net_and_float64_autograd():
    no, npv, A, ah, ch, S, eps = 37, 19, 5, [24, 16], [24, 16], 33, 1e-2
    g = torch.Generator().manual_seed(11)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    names = _names(3, 3)
    netA = _net(no, npv, A, ah, ch, "f32", 64, obs_norm=(eps, None))
    netB = _net(no, npv, A, ah, ch, "f32", 64)
    for net in (netA, netB):
        net.load_state_dict(dict(zip(names, p.tensors())))
    means, variances = _planted_general((no, npv), eps, g)
    (mfa, sfa), (mfc, sfc) = _plant(netA, means, variances)
    assert np.abs(mfa * sfa).max() > 2.9 and np.abs(mfa * sfa).max() <= 3.0 + 1e-5 and (np.asarray(variances[0]) == 0).sum() == 1
    e32 = float(np.float32(eps))
    x, xp = _raw_rows(S, means[0], variances[0], e32, g), _raw_rows(S, means[1], variances[1], e32, g)
    xn64, xpn64 = ON.normalise(x, mfa, sfa), ON.normalise(xp, mfc, sfc)
    xn, xpn = torch.from_numpy(xn64.astype(np.float32)), torch.from_numpy(xpn64.astype(np.float32))
    # the effective biases against the float64 restatement
    for i, (W, b, m, s) in enumerate(((p.actor[0][0], p.actor[0][1], mfa, sfa), (p.critic[0][0], p.critic[0][1], mfc, sfc))):
        _, want, scale = ON.fold(W.numpy(), b.numpy(), m, s, "f32")
        got = netA.norm_view("bias", i).cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= 2.0 ** -23 * (np.abs(b.numpy()) + scale)).all()
    # forward: A on raw rows, B on normalised rows, float64 on the float64 normalised rows
    pd = P.Params(FB.dbl(p.actor), FB.dbl(p.critic), p.std.double())
    with torch.no_grad():
        mu64, v64 = P.mlp_forward(torch.from_numpy(xn64), pd.actor), P.mlp_forward(torch.from_numpy(xpn64), pd.critic)
    muA, vA = netA.forward(0, torch.from_numpy(x).cuda()).cpu(), netA.forward(1, torch.from_numpy(xp).cuda()).cpu()
    muB, vB = netB.forward(0, xn.cuda()).cpu(), netB.forward(1, xpn.cuda()).cpu()
    for what, a, b in (("mu A:B", muA, muB), ("V A:B", vA, vB), ("mu A:f64", muA, mu64), ("V A:f64", vA, v64), ("mu B:f64", muB, mu64), ("V B:f64", vB, v64)):
        err = _rel_err(a.numpy(), b.numpy())
        print("%s %.3e" % (what, err))
        assert err <= F32_FWD_BAR, (what, err)
    # gradients of the master parameters
    rest = _columns_for(p, torch.from_numpy(xn64), torch.from_numpy(xpn64), A, g)
    idx = torch.randperm(S, generator=g)
    _grad(netA, torch.from_numpy(x), torch.from_numpy(xp), rest, idx, unfold=True)
    _grad(netB, xn, xpn, rest, idx, unfold=False)
    leaves = [t.clone().requires_grad_(True) for t in pd.tensors()]
    it = iter(leaves[1:])
    p64 = P.Params([(next(it), next(it)) for _ in range(3)], [(next(it), next(it)) for _ in range(3)], leaves[0])
    sel = [torch.from_numpy(xn64)[idx], torch.from_numpy(xpn64)[idx]] + [t[idx].double() for t in rest]
    P.ppo_loss_and_grads(p64, *sel)["loss"].backward()
    gA, gB = netA.grad_views(), netB.grad_views()
    for k, leaf in zip(names, leaves):
        ref = leaf.grad.numpy()
        ea, eb, eab = _rel_err(gA[k].cpu().numpy(), ref), _rel_err(gB[k].cpu().numpy(), ref), _rel_err(gA[k].cpu().numpy(), gB[k].cpu().numpy())
        print("%-18s A:f64 %.3e  B:f64 %.3e  A:B %.3e" % (k, ea, eb, eab))
        assert ea <= F32_GRAD_BAR and eb <= F32_GRAD_BAR and eab <= F32_GRAD_BAR, (k, ea, eb, eab)


def test_fold_f32_with_the_auxiliary_head():
    """All three nets fold: the auxiliary (denoising) head reads the actor's rows under the ACTOR's statistics, has an effective bias of
    its own, its first-layer gradient is unfolded with the others, and its regression targets -- columns of the privileged row -- stay
    raw.  Net A (statistics, raw rows) against plain net B (normalised rows) and float64 autograd, at the bars of the test above.  eps = 0,
    and the target columns carry mean 0, var 1 (scale exactly 1), so that B's normalised privileged rows hold the same targets."""
    no, npv, A, ah, ch, S, eps = 37, 19, 5, [24, 16], [24, 16], 33, 0.0
    aux, coef = ([20, 12], 4, 15), 0.5
    g = torch.Generator().manual_seed(12)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    head = P.Params.random(no, 8, aux[1], aux[0], [8], g).actor
    names = _names(3, 3) + ["denoiser.%d.%s" % (2 * l, k) for l in range(3) for k in ("weight", "bias")]
    tensors = p.tensors() + [t for wb in head for t in wb]
    netA = _net(no, npv, A, ah, ch, "f32", 64, obs_norm=(eps, None), aux=aux)
    netB = _net(no, npv, A, ah, ch, "f32", 64, aux=aux)
    assert list(netA.views) == names
    for net in (netA, netB):
        net.load_state_dict(dict(zip(names, tensors)))
    means, variances = [], []
    for k in (no, npv):
        var = (0.25 * 16.0 ** torch.rand(k, generator=g, dtype=torch.float64)).numpy()
        u = (torch.rand(k, generator=g, dtype=torch.float64) * 2 - 1).numpy()
        u[0] = 1.0
        means.append(3.0 * u * np.sqrt(var))
        variances.append(var)
    means[1][aux[2]:], variances[1][aux[2]:] = 0.0, 1.0
    (mfa, sfa), (mfc, sfc) = _plant(netA, means, variances)
    assert np.array_equal(sfc[aux[2]:], np.ones(aux[1], np.float32)) and not mfc[aux[2]:].any() and np.abs(mfa * sfa).max() > 2.9
    x, xp = _raw_rows(S, means[0], variances[0], 0.0, g), _raw_rows(S, means[1], variances[1], 0.0, g)
    xn64, xpn64 = ON.normalise(x, mfa, sfa), ON.normalise(xp, mfc, sfc)
    assert np.array_equal(xpn64[:, aux[2]:], xp[:, aux[2]:].astype(np.float64))          # the targets: raw on both sides
    xn, xpn = torch.from_numpy(xn64.astype(np.float32)), torch.from_numpy(xpn64.astype(np.float32))
    # the head's effective bias: the actor's statistics, the head's own first layer
    _, want, scale = ON.fold(head[0][0].numpy(), head[0][1].numpy(), mfa, sfa, "f32")
    got = netA.norm_view("bias", 2).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2.0 ** -23 * (np.abs(head[0][1].numpy()) + scale)).all()
    h64 = FB.dbl(head)
    with torch.no_grad():
        y64 = P.mlp_forward(torch.from_numpy(xn64), h64)
    yA, yB = netA.forward(2, torch.from_numpy(x).cuda()).cpu(), netB.forward(2, xn.cuda()).cpu()
    for what, a, b in (("head A:B", yA, yB), ("head A:f64", yA, y64), ("head B:f64", yB, y64)):
        err = _rel_err(a.numpy(), b.numpy())
        print("%s %.3e" % (what, err))
        assert err <= F32_FWD_BAR, (what, err)
    rest = _columns_for(p, torch.from_numpy(xn64), torch.from_numpy(xpn64), A, g)
    idx = torch.randperm(S, generator=g)
    _grad(netA, torch.from_numpy(x), torch.from_numpy(xp), rest, idx, unfold=True, aux_coef=coef)
    _grad(netB, xn, xpn, rest, idx, unfold=False, aux_coef=coef)
    pd = P.Params(FB.dbl(p.actor), FB.dbl(p.critic), p.std.double())
    leaves = [t.clone().requires_grad_(True) for t in pd.tensors()] + [t.clone().requires_grad_(True) for wb in h64 for t in wb]
    it = iter(leaves[1:])
    p64 = P.Params([(next(it), next(it)) for _ in range(3)], [(next(it), next(it)) for _ in range(3)], leaves[0])
    hd = [(next(it), next(it)) for _ in range(3)]
    X, XP = torch.from_numpy(xn64)[idx], torch.from_numpy(xpn64)[idx]
    loss = P.ppo_loss_and_grads(p64, X, XP, *[t[idx].double() for t in rest])["loss"]
    loss = loss + coef * ((P.mlp_forward(X, hd) - XP[:, aux[2]:]) ** 2).mean()
    loss.backward()
    gA, gB = netA.grad_views(), netB.grad_views()
    for k, leaf in zip(names, leaves):
        ref = leaf.grad.numpy()
        ea, eb, eab = _rel_err(gA[k].cpu().numpy(), ref), _rel_err(gB[k].cpu().numpy(), ref), _rel_err(gA[k].cpu().numpy(), gB[k].cpu().numpy())
        print("%-18s A:f64 %.3e  B:f64 %.3e  A:B %.3e" % (k, ea, eb, eab))
        assert ea <= F32_GRAD_BAR and eb <= F32_GRAD_BAR and eab <= F32_GRAD_BAR, (k, ea, eb, eab)
    assert float(gA["denoiser.0.weight"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. fold, fused bf16 path
XB = (705, 219, 12, [512, 256, 128], [768, 256, 128])
XB_NAMES = _names(4, 4)


def _xb_pair(eps, g):
    p = P.Params.random(*XB, g)
    p.std = torch.rand(12, generator=g) * 0.5 + 0.75
    netA = _net(*XB, "bf16", 128, obs_norm=(eps, None))
    netB = _net(*XB, "bf16", 128)
    assert netA.shadow_ld(0) > 0 and netB.shadow_ld(0) > 0, "not the fused bf16 path"
    for net in (netA, netB):
        net.load_state_dict(dict(zip(XB_NAMES, p.tensors())))
    return p, netA, netB


def test_fold_bf16_fused_power_of_two_scales_are_bit_identical():
    """eps = 0, mean = 0, var = 4^k with k in -2 .. 2 per column: s = 2^-k exactly, so T(w s) = T(w) s, the effective bias is b, and net A on
    rows x computes, product by product, what plain net B computes on rows x o s.  policy_act, critic_values, the unfolded flat gradient,
    and the parameters and Adam moments after ppo_apply are compared bit for bit."""
    S = 65
    g = torch.Generator().manual_seed(21)
    p, netA, netB = _xb_pair(0.0, g)
    ks = [(torch.arange(K) % 5 - 2).double() for K in (705, 219)]
    (mfa, sfa), (mfc, sfc) = _plant(netA, [np.zeros(705), np.zeros(219)], [(4.0 ** k).numpy() for k in ks])
    assert np.array_equal(sfa, (2.0 ** -ks[0]).numpy().astype(np.float32)) and np.array_equal(sfc, (2.0 ** -ks[1]).numpy().astype(np.float32))
    assert not mfa.any() and not mfc.any()
    for i, b in enumerate((p.actor[0][1], p.critic[0][1])):
        assert np.array_equal(netA.norm_view("bias", i).cpu().numpy(), b.numpy())
    x, xp = torch.randn(S, 705, generator=g) * 2, torch.randn(S, 219, generator=g) * 2
    xs, xps = x * torch.from_numpy(sfa), xp * torch.from_numpy(sfc)          # exact: powers of two
    z = torch.randn(S, 12, generator=g).cuda()
    oA, oB = netA.act(x.cuda(), xp.cuda(), z=z), netB.act(xs.cuda(), xps.cuda(), z=z)
    for k in ("actions", "mu", "sigma", "logp", "values"):
        assert _same_bits(oA[k], oB[k]), k
    vA, vB = torch.empty(S, device="cuda"), torch.empty(S, device="cuda")
    netA.critic_values(xp.cuda().contiguous(), vA)
    netB.critic_values(xps.cuda().contiguous(), vB)
    assert _same_bits(vA, vB) and _same_bits(netA.forward(0, x.cuda()), netB.forward(0, xs.cuda()))
    rest = _columns_for(p, xs, xps, 12, g, quant=FB.q64)
    idx = torch.randperm(S, generator=g)
    ppo, _ = _grad(netA, x, xp, rest, idx, unfold=True)
    _grad(netB, xs, xps, rest, idx, unfold=False)
    assert float(netA.grads.abs().max()) > 0 and _same_bits(netA.grads_ext, netB.grads_ext)
    for net in (netA, netB):
        net.ppo_apply(ppo)
    torch.cuda.synchronize()
    for a, b in ((netA.params, netB.params), (netA.adam_m, netB.adam_m), (netA.adam_v, netB.adam_v), (netA.opt_state, netB.opt_state)):
        assert _same_bits(a, b)
    assert not torch.equal(netA.params.cpu(), torch.cat([t.flatten() for t in p.tensors()]))       # the step moved them
    # ... and the step refolded: the forwards still agree bit for bit on the new parameters
    assert _same_bits(netA.forward(0, x.cuda()), netB.forward(0, xs.cuda())) and _same_bits(netA.forward(1, xp.cuda()), netB.forward(1, xps.cuda()))


def test_fold_bf16_fused_general_state_against_the_bf16_operand_oracle():
    """Non-zero means (|m| s up to 3, one var = 0 column), eps = 1e-2: the forward and the unfolded gradient against the float64
    bf16-operand oracle fed the FOLDED first layers (W o s in fp32 -- the oracle rounds it to bf16 as the operand copy is -- and b'),
    its first-layer weight gradients unfolded in float64; tests/fused_batch_common.py's 5e-3 bar, rel-L2 per tensor."""
    S, eps = 65, 1e-2
    g = torch.Generator().manual_seed(22)
    p, netA, _ = _xb_pair(eps, g)
    means, variances = _planted_general((705, 219), eps, g)
    (mfa, sfa), (mfc, sfc) = _plant(netA, means, variances)
    e32 = float(np.float32(eps))
    x, xp = _raw_rows(S, means[0], variances[0], e32, g), _raw_rows(S, means[1], variances[1], e32, g)
    folded = p.clone()
    for i, (layers, m, s) in enumerate(((folded.actor, mfa, sfa), (folded.critic, mfc, sfc))):
        W, b = layers[0]
        Wop, want, scale = ON.fold(W.numpy(), b.numpy(), m, s, "bf16")
        got = netA.norm_view("bias", i).cpu().numpy()
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * (np.abs(b.numpy()) + scale)).all()
        layers[0] = (torch.from_numpy(ON.operand(W.numpy(), s, "f32")), torch.from_numpy(got))
    fd = P.Params(FB.dbl(folded.actor), FB.dbl(folded.critic), p.std.double())
    X, XP = torch.from_numpy(x), torch.from_numpy(xp)
    with torch.no_grad():
        mu64, v64 = P.mlp_forward(X.double(), fd.actor, quant=FB.q64), P.mlp_forward(XP.double(), fd.critic, quant=FB.q64)
    emu, ev = FB.rel_l2(netA.forward(0, X.cuda()).cpu(), mu64), FB.rel_l2(netA.forward(1, XP.cuda()).cpu(), v64)
    print("forward rel-L2: mu %.3e  V %.3e" % (emu, ev))
    assert emu <= FB.BF16_OPERAND_TOL and ev <= FB.BF16_OPERAND_TOL
    rest = _columns_for(folded, X, XP, 12, g, quant=FB.q64)
    idx = torch.randperm(S, generator=g)
    _grad(netA, X, XP, rest, idx, unfold=True)
    with torch.no_grad():
        want = P.ppo_loss_and_grads(fd, X[idx].double(), XP[idx].double(), *[t[idx].double() for t in rest], quant=FB.q64)["grads"]
    ref = dict(zip(XB_NAMES, [t.numpy() for t in want.tensors()]))
    ref["actor.0.weight"] = ON.unfold(ref["actor.0.weight"], ref["actor.0.bias"], mfa, sfa)
    ref["critic.0.weight"] = ON.unfold(ref["critic.0.weight"], ref["critic.0.bias"], mfc, sfc)
    gA = netA.grad_views()
    for k in XB_NAMES:
        err = FB.rel_l2(gA[k].cpu(), torch.from_numpy(np.asarray(ref[k])))
        print("%-18s rel-L2 %.3e" % (k, err))
        assert err <= FB.BF16_OPERAND_TOL, (k, err)


# ------------------------------------------------------------------------------------------------ 4. off is off
@pytest.mark.parametrize("shape", ["f32_ragged", "bf16_fused"])
def test_identity_statistics_change_no_bit_of_two_optimiser_steps(shape):
    """A block at its initial state with eps = 0, until = 0 (mean 0, scale 1 / (1 + 0) = 1, no merge ever) against a net without the
    block, both with grad_norm_ready = 0: two ppo_grad (+ unfold) / ppo_apply steps -- with a normaliser step in between, which `until`
    turns into a no-op -- leave parameters, Adam moments and optimiser scalars bit-identical."""
    from hgym import make_batch
    no, npv, A, ah, ch, prec, S = (37, 19, 5, [24, 16], [24, 16], "f32", 33) if shape == "f32_ragged" else XB + ("bf16", 65)
    g = torch.Generator().manual_seed(31)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    names = _names(len(ah) + 1, len(ch) + 1)
    nets = [_net(no, npv, A, ah, ch, prec, 128), _net(no, npv, A, ah, ch, prec, 128, obs_norm=(0.0, 0))]
    assert nets[0].struct.norm is None and nets[1].struct.norm is not None
    for net in nets:
        net.load_state_dict(dict(zip(names, p.tensors())))
    assert float(nets[1].norm_view("scale_f", 0).min()) == 1.0 == float(nets[1].norm_view("scale_f", 1).max())
    x, xp = torch.randn(S, no, generator=g) * 2, torch.randn(S, npv, generator=g) * 2
    rest = _columns_for(p, x, xp, A, g, quant=FB.q64 if prec == "bf16" else None)
    for step in range(2):
        idx = torch.randperm(S, generator=g)
        for net in nets:
            ppo, _ = _grad(net, x, xp, rest, idx, unfold=net.obs_norm is not None)
            net.ppo_apply(ppo)
        assert _same_bits(nets[0].grads_ext, nets[1].grads_ext)
        nets[1].norm_accumulate(x.cuda(), xp.cuda())
        nets[1].norm_merge()          # count 0 >= until 0: skipped
        torch.cuda.synchronize()
        assert [c for _, _, c in _state(nets[1])] == [0.0, 0.0]
        for what in ("params", "adam_m", "adam_v", "opt_state"):
            assert _same_bits(getattr(nets[0], what), getattr(nets[1], what)), (step, what)
    assert float(nets[0].opt_state[L.OPT_STEP]) == 2.0
    assert _same_bits(nets[0].forward(0, x.cuda()), nets[1].forward(0, x.cuda()))
