"""Shared by tests/test_mirror_smooth.py (CPU) and the -m gpu tests of hgym_ppo_grad_smooth_mirror: the mirror loss
and the smoothness regulariser in one actor head, on top of update_options_common's float64 reference.

  make_case   smoothness_common.make_case (stored rows (T + 1) N, idx over the first T N, planted dones, a per-column noise_std) with every
              column doubled by update_options_common.mirror_columns -- [rows | mirrored rows], 2 (T + 1) N stored rows -- and
              pair = idx + (T + 1) N: every drawn row's partner lies in the mirrored half, no mirrored row is drawn (the mirror loss
              without augmentation), the successor idx + N stays in the original half.
  reference   written from the definition, not from the kernels:
                  L = L_ppo + c_m / (B A) sum |mu - M_a tm|^2 + lamT / (B A) sum w |mu - tT|^2 + lamS / (B A) sum |mu - tS|^2
              The partner rows, the successor rows and the perturbed rows go through the SAME bodies with the SAME quant as the rows
              themselves; the three targets are detached; autograd differentiates the three terms with respect to mu, the result joins
              the head's d_mu ahead of the actor's backward.  `near` = the perturbed rows (the device's own, or S.perturb's).
              -> U.reference's dict plus mirror (the plain MSE), smooth (temporal MSE, spatial MSE, sum of the weights), terms (each
              term's own d mu).
  WRONG       deliberately wrong variants: a term left out (drop=...), the action table not applied (table="identity"), w ignored
              (masked=False), a target not detached (detach=False, all three at once or one by one with detach_only)."""
import functools

import numpy as np
import torch

import layer_path_common as LP
import loss_head_common as H
import mirror_loss_common as M
import obs_norm_common as ON
import smoothness_common as S
import update_options_common as U

# The smoothness coefficients are smoothness_common's.  The mirror coefficient is four times mirror_loss_common's 0.5: beside two terms of
# weight 8 and 16 a term of weight 0.5 moves the actor's gradient by less than SENSITIVITY bars on the bf16 paths, and a reference that
# cannot see a term cannot hold a kernel to it (tests/test_mirror_smooth.py shows that every wrong variant is told apart with these).
COEF, LAM_T, LAM_S = 4.0 * M.COEF, S.LAM_T, S.LAM_S
WRONG = (dict(drop="mirror"), dict(drop="temporal"), dict(drop="spatial"), dict(table="identity"), dict(masked=False), dict(detach=False),
         dict(detach=False, detach_only="mirror"), dict(detach=False, detach_only="temporal"), dict(detach=False, detach_only="spatial"))


# A second fused shape for the head's other staging form: an actor whose update tile leaves LESS than the 9 600 bytes the head stages its
# targets in (hgym_fused.hpp: FB_MIRROR_LDS + FB_SMOOTH_LDS), so the launch runs with stage = 0 and the head reads them from memory.  Among
# the shapes fused_supported() accepts only actors with ONE action come that close to the 160 KiB (their tile is the critic's:
# 768-256-128 asks for 157 568 bytes, 6 272 free; tests/test_mirror_smooth_gpu.py confirms both figures on the host).  XBot-L's actor
# (512-256-128, 12 actions) asks for 133 504 and stages.  The path's name is not "f32-layer": quant, bars and metric are the bf16 paths'.
TIGHT = "bf16-fused-tight"
U.SHAPES.setdefault(TIGHT, dict(net=(705, 219, 1, [768, 256, 128], [768, 256, 128]), aux=([512, 256, 128], 73, 219 - 73), S=130, B=97))
U.SUM_TOL.setdefault(TIGHT, U.SUM_TOL["bf16-fused"])
S.LAYOUT.setdefault(TIGHT, S.LAYOUT["bf16-fused"])
HEAD_LDS = 64 * 12 * 4 + 2 * 16 * 4 + 2 * 64 * 12 * 4 + 64 * 4      # 9 600
FB_LDS_LIMIT = 160 * 1024


def make_case(opts, seed=0, B=None, layout=None):
    """layout: (T, N) other than smoothness_common.LAYOUT's, for minibatches larger than its T N rows."""
    if layout is None:
        c = S.make_case(opts, seed=seed, B=B)
    else:      # smoothness_common.make_case at another (T, N)
        T, N = layout
        B = B or U.SHAPES[opts.path]["B"]
        assert N >= 3 and T >= 4 and T * N >= B
        c = U.make_case(opts, S=(T + 1) * N, B=B, seed=seed)
        g = torch.Generator().manual_seed(7000 + seed)
        idx = torch.randperm(T * N, generator=g)[:B].contiguous()
        dones = np.zeros(T * N, dtype=np.uint8)
        dones[idx.numpy()[::3]] = 1
        nxt, weight = S.successor(idx.numpy(), dones, N)
        c = dict(c, idx=idx, dones=dones, nxt=torch.from_numpy(nxt), weight=torch.from_numpy(weight), noise_std=S.noise_of(opts, c["stats"], g),
                 T=T, N=N, S=T * N, B=B)
    spec = M.spec_of(opts.path)
    rows = (c["T"] + 1) * c["N"]
    assert c["cols"][0].shape[0] == rows and int(c["idx"].max()) < c["T"] * c["N"]
    pair = (c["idx"] + rows).contiguous()
    return dict(c, cols=U.mirror_columns(c["cols"], spec), pair=pair, spec=spec, rows=rows)


@functools.lru_cache(maxsize=None)
def case_of(opts):
    o = opts._replace(shadow=False)
    return make_case(o, seed=U.MATRIX.index(o))


def reference(case, coef=COEF, lam_t=LAM_T, lam_s=LAM_S, near=None, drop=None, table=None, masked=True, detach=True, detach_only=None, ppo=None):
    opts, params, stats, cols, idx, pair = case["opts"], case["params"], case["stats"], case["cols"], case["idx"], case["pair"]
    ppo = ppo or case["ppo"]
    dtype = torch.float64
    fwd, bwd = LP.restated(opts.activation)
    q = U.quant_of(opts)
    nets, ms = U.bodies(opts, params, stats, dtype)
    sel = [t[idx].to(dtype) for t in cols]
    X, XP = sel[0], sel[1]
    if near is None:
        near = S.clean_near(case)
    A = cols[2].shape[1]
    src, sign = (list(range(A)), [1.0] * A) if table == "identity" else (case["spec"].act_src, case["spec"].act_sign)
    src, sign = torch.tensor(src, dtype=torch.int64), torch.tensor(sign, dtype=dtype)
    with torch.no_grad():
        mu, a_acts, a_pres = fwd(X, nets["actor"], keep=True, quant=q)
        v, c_acts, c_pres = fwd(XP, nets["critic"], keep=True, quant=q)
        mu_p, p_acts, p_pres = fwd(cols[0][pair].to(dtype), nets["actor"], keep=True, quant=q)
        mu_n, n_acts, n_pres = fwd(cols[0][case["nxt"]].to(dtype), nets["actor"], keep=True, quant=q)
        mu_s, s_acts, s_pres = fwd(near.to(dtype), nets["actor"], keep=True, quant=q)
        y = target = None
        if opts.aux:
            y, x_acts, x_pres = fwd(X, nets["denoiser"], keep=True, quant=q)
            target = XP[:, XP.shape[1] - y.shape[1]:]
    p_name = "log_std" if opts.std == "log" else "std"
    hd = U.head(opts, sel[2:], mu, v.squeeze(-1), y, target, params[p_name].to(dtype), ppo)
    B = mu.shape[0]
    cm, lt, ls = (0.0 if drop == k else float(H.f32(c)) for k, c in (("mirror", coef), ("temporal", lam_t), ("spatial", lam_s)))
    w = case["weight"].to(dtype) if masked else torch.ones(B, dtype=dtype)
    m = mu.detach().clone().requires_grad_()
    leaves = dict(mirror=mu_p.detach().clone().requires_grad_(), temporal=mu_n.detach().clone().requires_grad_(),
                  spatial=mu_s.detach().clone().requires_grad_())
    through = lambda k: not detach and detach_only in (None, k)      # the gradient flows through this target
    tg = {k: (t if through(k) else t.detach()) for k, t in leaves.items()}
    tm = sign * tg["mirror"][:, src]
    se_m = ((m - tm) ** 2).sum()
    se_t = (w[:, None] * (m - tg["temporal"]) ** 2).sum()
    se_s = ((m - tg["spatial"]) ** 2).sum()
    parts = dict(mirror=cm * se_m / (B * A), temporal=lt * se_t / (B * A), spatial=ls * se_s / (B * A))
    terms = {k: torch.autograd.grad(p, m, retain_graph=True)[0] for k, p in parts.items()}
    d_mu = ((hd["d_mu"] + terms["mirror"]) + terms["temporal"]) + terms["spatial"]
    with torch.no_grad():
        got = {"actor": bwd(d_mu, nets["actor"], a_acts, a_pres, quant=q),
               "critic": bwd(hd["d_val"].unsqueeze(1), nets["critic"], c_acts, c_pres, quant=q)}
    for k, (acts, pres) in (("mirror", (p_acts, p_pres)), ("temporal", (n_acts, n_pres)), ("spatial", (s_acts, s_pres))):
        if through(k):
            gx = torch.autograd.grad(parts[k], leaves[k], retain_graph=True)[0]
            with torch.no_grad():
                extra = bwd(gx, nets["actor"], acts, pres, quant=q)
            got["actor"] = [(gW + eW, gb + eb) for (gW, gb), (eW, eb) in zip(got["actor"], extra)]
    with torch.no_grad():
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
    return dict(grads=grads, sums=sums, d_val=hd["d_val"], d_mu=d_mu, mirror=float(se_m.detach()) / (B * A),
                smooth=(float(se_t.detach()) / (B * A), float(se_s.detach()) / (B * A), float(w.sum())), terms=terms, mu=mu,
                targets=dict(mirror=tm.detach(), temporal=mu_n, spatial=mu_s), weight=w)
