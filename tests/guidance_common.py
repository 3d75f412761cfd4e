"""Shared by tests/test_guidance.py (CPU) and tests/test_guidance_gpu.py (-m gpu): the frozen teacher's cloning term (hgym_guide_schedule,
hgym_ppo_grad_guide) on top of update_options_common's float64 reference.

  make_case   U.make_case plus `teacher_mu`: the mean of a SECOND, differently seeded parameter set on all S stored rows, through the same
              float64 bodies (same activation, same quant, same statistics), rounded to fp32 once -- the column the device reads.  Two
              independently drawn nets: mu - t is of the size of mu itself.
  schedule    the Python twin of hgym_guide_schedule is hgym.guide_schedule_coef; SCHED is the schedule of every gradient case (linear from
              COEF at update 0 to 0 at update FINAL) and K the update count the cases are taken at, so that the coefficients of updates K and
              K + 1 differ by a quarter of COEF.
  reference   U.reference with c / (B A) sum (mu - t[idx])^2 added to the head's loss, the target detached (it is data).  Switches, each a
              way an implementation could be wrong: per_action=False (1 / B instead of 1 / (B A)), target_row="b" (the target taken at row b
              of the column instead of r_b = idx[b]), next_coef=True (the coefficient of update K + 1), sign=-1.0.
  COEF        8.0.  The mirror loss's 0.5 is too weak here: the teacher's mean varies little from row to row (a freshly drawn net's output is
              mostly its bias), so taking the target at row b instead of r_b moves d mu by a small share of the term, and the term itself
              must outweigh the PPO part of d mu before that share shows.  At 2.0 that variant moved the worst actor tensor of the bf16
              cases by 3.9 to 5.0 bars; at 8.0 every wrong variant clears SENSITIVITY (10) bars on every case of tests/test_guidance.py,
              the closest being the same variant at 15.0 bars on the fused ELU case (the test prints every figure)."""
import functools

import torch

import layer_path_common as LP
import loss_head_common as H
import obs_norm_common as ON
import update_options_common as U

COEF = 8.0
FINAL, K = 4, 1
WRONG = (dict(per_action=False), dict(target_row="b"), dict(next_coef=True), dict(sign=-1.0))
TEACHER_SEED = 424242


def sched(coef=COEF, final=FINAL):
    import hgym
    return hgym.make_guide_schedule("linear", coef, 0.0, 0, final)


def coef_at(k, coef=COEF):
    import hgym
    return hgym.guide_schedule_coef(sched(coef), k)


def make_case(opts, seed=0, B=None):
    """-> U.make_case's dict plus teacher_params and teacher_mu ((S, A) float32)."""
    c = U.make_case(opts, B=B, seed=seed)
    g = torch.Generator().manual_seed(TEACHER_SEED + seed)
    tp = U.make_params(opts, g)
    mu_t, _, _ = U.forward(opts, tp, c["stats"], c["cols"][0], c["cols"][1])
    return dict(c, teacher_params=tp, teacher_mu=mu_t.float().contiguous())


@functools.lru_cache(maxsize=None)
def case_of(opts):
    o = opts._replace(shadow=False)
    return make_case(o, seed=U.MATRIX.index(o))


def reference(case, c=None, per_action=True, target_row="r", next_coef=False, sign=1.0):
    """U.reference's dict with the term in it, plus guide = the plain MSE of the minibatch.  c: the coefficient (an fp32 value), by default
    the schedule's at update K."""
    opts, params, stats, cols, idx = case["opts"], case["params"], case["stats"], case["cols"], case["idx"]
    ppo = case["ppo"]
    dtype = torch.float64
    if c is None:
        c = coef_at(K + 1 if next_coef else K)
    fwd, bwd = LP.restated(opts.activation)
    q = U.quant_of(opts)
    nets, ms = U.bodies(opts, params, stats, dtype)
    sel = [t[idx].to(dtype) for t in cols]
    X, XP = sel[0], sel[1]
    with torch.no_grad():
        mu, a_acts, a_pres = fwd(X, nets["actor"], keep=True, quant=q)
        v, c_acts, c_pres = fwd(XP, nets["critic"], keep=True, quant=q)
        y = target = None
        if opts.aux:
            y, x_acts, x_pres = fwd(X, nets["denoiser"], keep=True, quant=q)
            target = XP[:, XP.shape[1] - y.shape[1]:]
    p_name = "log_std" if opts.std == "log" else "std"
    hd = U.head(opts, sel[2:], mu, v.squeeze(-1), y, target, params[p_name].to(dtype), ppo)
    B, A = mu.shape
    t = (case["teacher_mu"][idx] if target_row == "r" else case["teacher_mu"][:B]).to(dtype)
    m = mu.detach().clone().requires_grad_()
    se = ((m - t) ** 2).sum()
    term = sign * float(H.f32(c)) * se / (B * A if per_action else B)
    g_m, = torch.autograd.grad(term, [m])
    d_mu = hd["d_mu"] + g_m
    with torch.no_grad():
        got = {"actor": bwd(d_mu, nets["actor"], a_acts, a_pres, quant=q),
               "critic": bwd(hd["d_val"].unsqueeze(1), nets["critic"], c_acts, c_pres, quant=q)}
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
    return dict(grads=grads, sums=sums, d_val=hd["d_val"], d_mu=d_mu, guide=float(se.detach()) / (B * A), mu=mu, t=t)
