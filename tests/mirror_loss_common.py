"""Shared by tests/test_mirror_loss.py (CPU) and tests/test_mirror_loss_gpu.py (-m gpu): the mirror loss of left-right symmetry
(PPO.mirror_loss_coef, HgymPPOConfig.mirror_coef) on top of update_options_common's float64 reference.

  reference   update_options_common.reference with the term added to the head's loss: the partner rows go through the SAME bodies with
              the SAME quant as the rows themselves, t = M_a(mu(partner)) is detached, L_m = coef * mean_b mean_j (mu - t)^2 joins the
              loss, d L_m / d mu joins the head's d_mu ahead of the actor's backward.  Three switches exist for the CPU test only, each a
              way the implementation could be wrong: detach=False (the gradient also flows through the target), the identity table
              instead of MirrorSpec's, per_action=False (1 / B instead of 1 / (B A)).
  make_case   U.make_case at half the path's stored rows, doubled by U.mirror_columns -- [rows | mirrored rows], U.SHAPES[path]["S"] stored
              rows in all -- and an index slice of U.SHAPES[path]["B"] rows drawn over both halves (more than half of the rows: some row is
              drawn together with its own partner).
  COEF        the coefficient of every case: 0.5 (rsl_rl's scale for mirror_loss_coeff; tests/test_mirror_loss.py shows that all four
              sensitivity cases hold with it)."""
import functools

import torch

import layer_path_common as LP
import loss_head_common as H
import obs_norm_common as ON
import update_options_common as U

COEF = 0.5


def involution_spec(no, npv, A, g):
    """A random signed involution MirrorSpec for any widths: columns paired off at random (an odd one left fixed), one sign per pair."""
    from humanoid.utils.symmetry import MirrorSpec

    def table(w):
        order = torch.randperm(w, generator=g).tolist()
        src, sign = list(range(w)), [1] * w
        for k in range(0, w - 1, 2):
            a, b = order[k], order[k + 1]
            s = 1 if float(torch.rand(1, generator=g)) < 0.5 else -1
            src[a], src[b], sign[a], sign[b] = b, a, s, s
        if w % 2:
            sign[order[-1]] = -1
        return src, sign
    return MirrorSpec(*table(no), *table(npv), *table(A))


@functools.lru_cache(maxsize=None)
def spec_of(path):
    """XBot-L's tables where the net has XBot-L's widths, a random involution for the small fp32 net (5 actions)."""
    no, npv, A = U.SHAPES[path]["net"][:3]
    if (no, npv, A) == (705, 219, 12):
        return U.xbot_l_spec()
    return involution_spec(no, npv, A, torch.Generator().manual_seed(97))


def make_case(opts, seed=0, B=None):
    """-> U.make_case's dict with cols = the doubled columns, idx over both halves, pair = every drawn row's partner, spec, half."""
    sh = U.SHAPES[opts.path]
    half, B = sh["S"] // 2, B or sh["B"]
    c = U.make_case(opts, S=half, B=half - 1, seed=seed)
    spec = spec_of(opts.path)
    g = torch.Generator().manual_seed(5000 + seed)
    idx = torch.randperm(2 * half, generator=g)[:B].contiguous()
    if B > half:
        assert len(set((idx % half).tolist())) < B      # a row and its own partner are both drawn
    pair = ((idx + half) % (2 * half)).contiguous()
    return dict(c, cols=U.mirror_columns(c["cols"], spec), idx=idx, pair=pair, spec=spec, half=half, S=2 * half, B=B)


@functools.lru_cache(maxsize=None)
def case_of(opts):
    o = opts._replace(shadow=False)
    return make_case(o, seed=U.MATRIX.index(o))


def reference(case, coef=COEF, detach=True, table=None, per_action=True, ppo=None, cols=None, idx=None, pair=None):
    """U.reference's dict with the mirror term in it, plus mirror = the minibatch's plain MSE (what mirror_sums[0] receives).  coef 0:
    U.reference itself (mirror = the MSE all the same)."""
    opts, params, stats = case["opts"], case["params"], case["stats"]
    cols, idx, pair = cols or case["cols"], case["idx"] if idx is None else idx, case["pair"] if pair is None else pair
    ppo = ppo or case["ppo"]
    src, sign = table or (case["spec"].act_src, case["spec"].act_sign)
    src, sign = torch.tensor(src, dtype=torch.int64), torch.tensor(sign, dtype=torch.float64)
    dtype = torch.float64
    fwd, bwd = LP.restated(opts.activation)
    q = U.quant_of(opts)
    nets, ms = U.bodies(opts, params, stats, dtype)
    sel = [t[idx].to(dtype) for t in cols]
    X, XP = sel[0], sel[1]
    with torch.no_grad():
        mu, a_acts, a_pres = fwd(X, nets["actor"], keep=True, quant=q)
        v, c_acts, c_pres = fwd(XP, nets["critic"], keep=True, quant=q)
        mu_p, p_acts, p_pres = fwd(cols[0][pair].to(dtype), nets["actor"], keep=True, quant=q)      # same bodies, same quant
        y = target = None
        if opts.aux:
            y, x_acts, x_pres = fwd(X, nets["denoiser"], keep=True, quant=q)
            target = XP[:, XP.shape[1] - y.shape[1]:]
    p_name = "log_std" if opts.std == "log" else "std"
    hd = U.head(opts, sel[2:], mu, v.squeeze(-1), y, target, params[p_name].to(dtype), ppo)
    B, A = mu.shape
    c64 = float(H.f32(coef))
    m = mu.detach().clone().requires_grad_()
    mp = mu_p.detach().clone().requires_grad_()
    t = sign * mp[:, src]
    if detach:
        t = t.detach()
    se = ((m - t) ** 2).sum(dim=-1)
    mse = se.mean() / A
    term = c64 * (mse if per_action else se.mean())
    g_m, g_p = torch.autograd.grad(term, [m, mp], allow_unused=True)
    d_mu = hd["d_mu"] + g_m
    with torch.no_grad():
        got = {"actor": bwd(d_mu, nets["actor"], a_acts, a_pres, quant=q),
               "critic": bwd(hd["d_val"].unsqueeze(1), nets["critic"], c_acts, c_pres, quant=q)}
        if not detach:
            extra = bwd(g_p, nets["actor"], p_acts, p_pres, quant=q)
            got["actor"] = [(gW + eW, gb + eb) for (gW, gb), (eW, eb) in zip(got["actor"], extra)]
        if opts.aux:
            got["denoiser"] = bwd(hd["d_y_aux"], nets["denoiser"], x_acts, x_pres, quant=q)
    grads = {p_name: hd["d_std"]}
    for net, g in got.items():
        for l, (gW, gb) in enumerate(g):
            if l == 0 and opts.norm:
                mm, s = ms[1] if net == "critic" else ms[0]
                gW = torch.from_numpy(ON.unfold(gW.double().numpy(), gb.double().numpy(), mm, s)).to(dtype)
            grads["%s.%d.weight" % (net, 2 * l)], grads["%s.%d.bias" % (net, 2 * l)] = gW, gb
    sums = {k: hd[k] for k in ("surrogate", "value", "entropy", "kl", "aux", "surrogate_abs", "entropy_abs")}
    return dict(grads=grads, sums=sums, d_val=hd["d_val"], d_mu=d_mu, mirror=float(mse.detach()), mu=mu, target=t.detach())


def asymmetry(opts, params, stats, obs, obs_mirrored, spec):
    """mean (mu(s) - M_a mu(M s))^2 over rows and actions, float64, under the options' bodies."""
    priv = torch.zeros(obs.shape[0], U.SHAPES[opts.path]["net"][1])      # (the critic's rows: not looked at)
    mu, _, _ = U.forward(opts, params, stats, obs, priv)
    mu_m, _, _ = U.forward(opts, params, stats, obs_mirrored, priv)
    src, sign = torch.tensor(spec.act_src, dtype=torch.int64), torch.tensor(spec.act_sign, dtype=torch.float64)
    return float(((mu - sign * mu_m[:, src]) ** 2).mean())
