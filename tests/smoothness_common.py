"""Shared by tests/test_smoothness.py (CPU) and tests/test_smoothness_gpu.py (-m gpu): the smoothness regulariser on the policy's mean
(hgym_ppo_grad_smooth, HgymSmooth) on top of update_options_common's float64 reference.

  layout      stored rows are (T, N) plus the N rows of slot T: the observation column has (T + 1) N rows, the successor of flat row r is
              row r + N.  LAYOUT[path] = (T, N) with T N = update_options_common.SHAPES[path]["S"].
  make_case   U.make_case over (T + 1) N rows, an index slice over the first T N, `dones` planted by position in the minibatch (every third
              drawn row has ended: a third of the rows masked, both kinds in every 64-row tile), a per-column noise_std (a share of the
              column's spread, a few columns exactly 0).
  reference   U.reference with the two terms added to the head's loss: the successor rows and the perturbed rows go through the SAME
              bodies with the SAME quant as the rows themselves, both targets detached, the gradient joins the head's d_mu ahead of the
              actor's backward.  `near` = the perturbed rows (the device's own, or perturb() below).  Switches, each a way an
              implementation could be wrong: detach=False, per_action=False (1 / B instead of 1 / (B A)), masked=False (done rows keep
              their weight), successor="r+1", near_from_clean=True (the spatial target from the unperturbed row).
  perturb     hgym_perturb_rows restated with oracle/philox.py.
  LAM_T, LAM_S, NOISE_REL   the coefficients and the noise of every case; tests/test_smoothness.py shows that every switch moves some
              actor tensor by more than SENSITIVITY x the path's bar with them."""
import functools

import numpy as np
import torch

import layer_path_common as LP
import loss_head_common as H
import obs_norm_common as ON
import update_options_common as U
from oracle import philox as PH

LAM_T, LAM_S = 8.0, 16.0
NOISE_REL = (0.2, 0.5)      # noise_std[c] = u * (the column's spread), u uniform in this range
SEED = 0x5EEDF00D12345
SLOT_PERTURB = 128
LAYOUT = {"bf16-fused": (13, 10), "f32-layer": (10, 5), "bf16-layer": (13, 10)}
WRONG = (dict(detach=False), dict(per_action=False), dict(masked=False), dict(successor="r+1"), dict(near_from_clean=True))


def successor(idx, dones, N):
    """hgym_smooth_pairs restated in numpy: (idx + N, 0.0 where dones[idx] else 1.0)."""
    idx = np.asarray(idx, dtype=np.int64)
    return idx + np.int64(N), np.where(np.asarray(dones)[idx] != 0, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def normals(seed, step, rows, width):
    """z[m, c] of hgym_perturb_rows: normal c of the Philox block (seed, step, env word = rows[m]) from slot 128 on."""
    return PH.normals(seed, step, np.asarray(rows, dtype=np.int64).astype(np.uint32), SLOT_PERTURB, width)


def perturb(src_rows, noise_std, seed, step, rows):
    """src_rows (M, width) float32 + noise_std * z in one fused multiply-add (float64 product and sum of fp32 operands, one rounding);
    columns with noise_std == 0 copied."""
    x, ns = np.asarray(src_rows, dtype=np.float32), np.asarray(noise_std, dtype=np.float32)
    z = normals(seed, step, rows, x.shape[1])
    out = (x.astype(np.float64) + ns.astype(np.float64)[None, :] * z.astype(np.float64)).astype(np.float32)
    return np.where(ns[None, :] == 0, x, out)


def noise_of(opts, stats, g):
    no = U.SHAPES[opts.path]["net"][0]
    u = NOISE_REL[0] + (NOISE_REL[1] - NOISE_REL[0]) * torch.rand(no, generator=g, dtype=torch.float64).numpy()
    spread = np.sqrt(np.asarray(stats["var"][0], np.float64)) + stats["eps"] if opts.norm else np.ones(no)
    ns = (u * spread).astype(np.float32)
    ns[::7] = 0.0      # columns that must keep their bits
    return ns


def make_case(opts, seed=0, B=None):
    """-> U.make_case's dict with cols over (T + 1) N rows, idx over the first T N, dones (T N,) uint8, nxt / weight (the successor map),
    noise_std, T, N, S = T N."""
    T, N = LAYOUT[opts.path]
    assert N >= 3 and T >= 4 and T * N == U.SHAPES[opts.path]["S"]
    B = B or U.SHAPES[opts.path]["B"]
    c = U.make_case(opts, S=(T + 1) * N, B=B, seed=seed)
    g = torch.Generator().manual_seed(7000 + seed)
    idx = torch.randperm(T * N, generator=g)[:B].contiguous()
    dones = np.zeros(T * N, dtype=np.uint8)
    dones[idx.numpy()[::3]] = 1
    nxt, weight = successor(idx.numpy(), dones, N)
    return dict(c, idx=idx, dones=dones, nxt=torch.from_numpy(nxt), weight=torch.from_numpy(weight), noise_std=noise_of(opts, c["stats"], g),
                T=T, N=N, S=T * N, B=B)


def check_mask(case):
    """Between a quarter and three quarters of the drawn rows are masked, and every 64-row tile holds both kinds."""
    w = case["weight"].numpy()
    assert 0.25 <= float((w == 0).mean()) <= 0.75, float((w == 0).mean())
    for t0 in range(0, len(w), 64):
        tile = w[t0:t0 + 64]
        assert (tile == 0).any() and (tile == 1).any(), t0


@functools.lru_cache(maxsize=None)
def case_of(opts):
    o = opts._replace(shadow=False)
    return make_case(o, seed=U.MATRIX.index(o))


def clean_near(case, step=0):
    """The perturbed rows of the case's minibatch as perturb() gives them (the CPU test's; the GPU test feeds the device's own)."""
    idx = case["idx"].numpy()
    return torch.from_numpy(perturb(case["cols"][0][case["idx"]].numpy(), case["noise_std"], SEED, step, idx))


def reference(case, lam_t=LAM_T, lam_s=LAM_S, near=None, detach=True, per_action=True, masked=True, successor="r+N", near_from_clean=False,
              ppo=None):
    """U.reference's dict with the two terms in it, plus smooth = (the plain temporal MSE, the plain spatial MSE, sum of the weights)."""
    opts, params, stats, cols, idx = case["opts"], case["params"], case["stats"], case["cols"], case["idx"]
    ppo = ppo or case["ppo"]
    dtype = torch.float64
    fwd, bwd = LP.restated(opts.activation)
    q = U.quant_of(opts)
    nets, ms = U.bodies(opts, params, stats, dtype)
    sel = [t[idx].to(dtype) for t in cols]
    X, XP = sel[0], sel[1]
    nxt = case["nxt"] if successor == "r+N" else idx + 1
    if near is None:
        near = clean_near(case)
    Xn = cols[0][nxt].to(dtype)
    Xs = X if near_from_clean else near.to(dtype)
    with torch.no_grad():
        mu, a_acts, a_pres = fwd(X, nets["actor"], keep=True, quant=q)
        v, c_acts, c_pres = fwd(XP, nets["critic"], keep=True, quant=q)
        mu_n, n_acts, n_pres = fwd(Xn, nets["actor"], keep=True, quant=q)      # same bodies, same quant
        mu_s, s_acts, s_pres = fwd(Xs, nets["actor"], keep=True, quant=q)
        y = target = None
        if opts.aux:
            y, x_acts, x_pres = fwd(X, nets["denoiser"], keep=True, quant=q)
            target = XP[:, XP.shape[1] - y.shape[1]:]
    p_name = "log_std" if opts.std == "log" else "std"
    hd = U.head(opts, sel[2:], mu, v.squeeze(-1), y, target, params[p_name].to(dtype), ppo)
    B, A = mu.shape
    lt, ls = float(H.f32(lam_t)), float(H.f32(lam_s))
    w = case["weight"].to(dtype) if masked else torch.ones(B, dtype=dtype)
    m = mu.detach().clone().requires_grad_()
    tn = mu_n.detach().clone().requires_grad_()
    ts = mu_s.detach().clone().requires_grad_()
    tT, tS = (tn.detach(), ts.detach()) if detach else (tn, ts)
    seT = (w[:, None] * (m - tT) ** 2).sum()
    seS = ((m - tS) ** 2).sum()
    div = B * A if per_action else B
    term = lt * seT / div + ls * seS / div
    g_m, g_n, g_s = torch.autograd.grad(term, [m, tn, ts], allow_unused=True)
    d_mu = hd["d_mu"] + (g_m if g_m is not None else 0.0)
    with torch.no_grad():
        got = {"actor": bwd(d_mu, nets["actor"], a_acts, a_pres, quant=q),
               "critic": bwd(hd["d_val"].unsqueeze(1), nets["critic"], c_acts, c_pres, quant=q)}
        if not detach:
            for gx, acts, pres in ((g_n, n_acts, n_pres), (g_s, s_acts, s_pres)):
                extra = bwd(gx, nets["actor"], acts, pres, quant=q)
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
    smooth = (float(seT.detach()) / (B * A), float(seS.detach()) / (B * A), float(w.sum()))
    return dict(grads=grads, sums=sums, d_val=hd["d_val"], d_mu=d_mu, smooth=smooth, mu=mu, mu_next=mu_n, mu_near=mu_s)


def roughness(opts, params, stats, obs, obs_next, weight):
    """mean over undone rows and actions of |mu(s_t) - mu(s_t+1)|^2, float64, under the options' bodies (obs_next may be perturbed rows with
    weight all ones: the spatial roughness)."""
    priv = torch.zeros(obs.shape[0], U.SHAPES[opts.path]["net"][1])
    mu, _, _ = U.forward(opts, params, stats, obs, priv)
    mu_n, _, _ = U.forward(opts, params, stats, obs_next, priv)
    w = torch.as_tensor(weight, dtype=torch.float64)
    return float((w[:, None] * (mu - mu_n) ** 2).sum() / (w.sum() * mu.shape[1]))
