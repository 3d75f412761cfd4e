"""-m gpu: the PPO loss head of every update path, sample by sample, against float64 autograd (tests/loss_head_common.py: the probe
network, the reference, the case table, the tolerances and the reasoning behind them; tests/test_loss_head.py checks on the host that the
table holds what is relied on here).

Paths (each with the clipped and the unclipped value loss):
  f32           ppo_loss_kernel<float>                                    precision "f32"
  bf16-generic  ppo_loss_kernel<bf16>                                     "bf16" with HGYM_NO_FUSED=1
  fused-pre     fb_body's head, loss inputs pre-gathered into LDS         "bf16", shapes xbotl / narrow, A = 12
  fused-nopre   fb_body's head, both HBM branches                         shapes wide3 / g1 (A = 12), xbotl with every A != 12
  fused-shadow  the XB16 instantiation                                    fused-pre with the bf16 input shadows handed to make_batch

Per case and path, one hgym_ppo_grad on a gradient buffer pre-filled with NaN, and a second one that must leave the same bits:
  1. per sample: column i of the actor head weight gradient against g_mu[i], entry i of the critic head weight gradient against d_v[i];
     columns >= B exactly zero; everything finite although every storage row outside the index list is NaN;
  2. sums: both head bias gradients, the std gradient, opt_state[3], [4], [5] (+= sum / B) and [8] (= float(sum / B)): ppo_scalars_block;
  3. boundary cases: each sample equals one of the two float64 gradients (indicator in / out) in all its components; no sums;
  4. the hidden layers' weight gradients are zero outside their B x B block and finite inside.
Every failure of a path is collected and reported together with the sample's lane, so that a miss can be read from the residuals."""
import time

import pytest
import torch

import bf16_report as BR
import loss_head_common as H
from hgym import _lib as L

pytestmark = pytest.mark.gpu

MAX_BATCH = 256
FACTOR = H.GPU_FACTOR * H.K_REF

# id: (precision, HGYM_NO_FUSED, fused kernels expected, input shadows, shapes a case runs on)
PATHS = {
    "f32": ("f32", False, False, False, lambda c: ["xbotl"] if c["B"] <= 128 else ["g1"]),
    "bf16-generic": ("bf16", True, False, False, lambda c: ["xbotl"] if c["B"] <= 128 else ["g1"]),
    "fused-pre": ("bf16", False, True, False, lambda c: ["xbotl", "narrow"] if c["A"] == 12 and c["B"] <= 128 else []),
    "fused-nopre": ("bf16", False, True, False,
                    lambda c: (["g1"] + (["wide3"] if c["B"] <= 128 else [])) if c["A"] == 12 else ["xbotl"]),
    "fused-shadow": ("bf16", False, True, True, lambda c: ["xbotl", "narrow"] if c["A"] == 12 and c["B"] <= 128 else []),
}


def _net(shape, A, precision):
    from hgym import NetBuffers, make_net_config
    n_obs, n_priv, ah, ch = H.SHAPES[shape]
    return NetBuffers(make_net_config(n_obs, n_priv, A, ah, ch, precision, MAX_BATCH), "cuda", learning_rate=1e-3)


def _run(net, case, shape, clipped, shadow):
    """-> (gradient views on the CPU, opt_state after the first call)."""
    from hgym import make_ppo_config, make_batch
    n_obs, n_priv, ah, ch = H.SHAPES[shape]
    p, obs_rows, priv_rows = H.probe_params(n_obs, n_priv, case["A"], ah, ch, case["mu"], case["v"], case["std"])
    net.load_state_dict(dict(zip(list(net.views), p.tensors())))
    obs, priv = H.storage_inputs(case, n_obs, n_priv, obs_rows, priv_rows)
    c = case["cols"]
    cols = [t.cuda().contiguous() for t in (obs, priv, c["actions"], c["values"], c["adv"], c["returns"], c["logp"], c["mu_old"],
                                            c["sigma_old"])]
    idx = case["idx"].cuda()
    kw = {}
    if shadow:      # one-hot rows are exact in bf16; the pad columns of a selected row are zero, every other row is NaN
        for key, rows, n, which in (("obs_bf16", obs_rows, n_obs, 0), ("priv_bf16", priv_rows, n_priv, 1)):
            s = torch.full((case["S"], net.shadow_ld(which)), float("nan"), dtype=torch.bfloat16)
            s[case["idx"]] = 0.0
            s[case["idx"], :n] = rows.to(torch.bfloat16)
            kw[key] = s.cuda().contiguous()
    batch = make_batch(*cols, idx, **kw)
    ppo = make_ppo_config(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.001, clipped_value_loss=clipped)
    net.opt_state[L.OPT_KL_SUM:L.OPT_GRAD_SQNORM + 1] = 0.0
    net.grads_ext.fill_(float("nan"))
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    g1, o1 = net.grads_ext.clone(), net.opt_state.clone()
    net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    g2, o2 = net.grads_ext.clone(), net.opt_state.clone()
    same = torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(o2[[3, 4, 5]], 2.0 * o1[[3, 4, 5]]) and \
        torch.equal(o2[8], o1[8])
    return {k: v.cpu().double() for k, v in net.grad_views().items()}, o1.cpu(), same


def _check(tag, case, fused, bf16, g, opt, ref, un, fails, worst):
    B, A = case["B"], case["A"]

    def fail(msg):
        fails.append("%s: %s" % (tag, msg))

    for k, t in g.items():
        if not torch.isfinite(t).all():
            fail("%s: %d non-finite entries" % (k, int((~torch.isfinite(t)).sum())))
    # 1 / 3. per sample
    Wa, Wc = g["actor.6.weight"], g["critic.6.weight"]
    if Wa[:, B:].any() or Wc[:, B:].any():
        fail("head weight gradient not zero in columns >= B")
    ex_mu = H.mu_excess(Wa[:, :B].t(), ref, un, case["boundary"], FACTOR, bf16)
    ex_v = H.excess(Wc[0, :B], ref["d_v"], un["d_v"], FACTOR, bf16)
    for name, ex, got, want in (("g_mu", ex_mu, Wa[:, :B].t(), ref["g_mu"]), ("d_v", ex_v, Wc[0, :B].unsqueeze(-1), ref["d_v"].unsqueeze(-1))):
        worst["sample"] = max(worst["sample"], float(ex.max()))
        for i in torch.nonzero(ex > 1.0).flatten().tolist()[:6]:
            fail("%s sample %d (tile row %d, lane row %d, kind %s, adv %g, log ratio %.6f): %.3g x the bar; got %s want %s" % (
                name, i, i % 64, i % 16, case["kinds"][i], float(H.rows_of(case)["adv"][i]), float(ref["log_ratio"][i]), float(ex[i]),
                got[i].tolist(), want[i].tolist()))
    if not bf16:        # fp32 values: the error in units, next to K_REF
        strict = ~case["boundary"]
        if strict.any():
            worst["units"] = max(worst["units"], float(H.excess(Wa[:, :B].t(), ref["g_mu"], un["g_mu"], 1.0)[strict].max()),
                                 float(H.excess(Wc[0, :B], ref["d_v"], un["d_v"], 1.0).max()))
    # 2. sums
    if not case["boundary"].any():
        stored = bf16 and not fused       # rowsum_kernel sums the stored bf16 head gradient (loss_head_common.py)
        kl_sum = ref["kl"].sum()
        sums = (("actor.6.bias", g["actor.6.bias"], ref["g_mu"], un["g_mu"], stored, 0.0),
                ("critic.6.bias", g["critic.6.bias"][0], ref["d_v"], un["d_v"], stored, 0.0),
                ("std", g["std"], ref["g_sigma"], un["g_sigma"], False, 0.0),
                ("opt_state[OPT_SURROGATE_SUM] surrogate", opt[L.OPT_SURROGATE_SUM] * B, ref["surr"], un["surr"], False, 0.0),
                ("opt_state[OPT_VALUE_SUM] value loss", opt[L.OPT_VALUE_SUM] * B, ref["vl"], un["vl"], False, 0.0),
                ("opt_state[OPT_ENTROPY_SUM] entropy", opt[L.OPT_ENTROPY_SUM] * B, ref["ent"], un["ent"], False, 0.0),
                ("opt_state[OPT_KL_LAST] KL", opt[L.OPT_KL_LAST] * B, ref["kl"], un["kl"], False, H.U24 * float(kl_sum.abs())))     # stored as a float
        for name, got, terms, unit, st, extra in sums:
            want = terms.sum(0)
            bar = H.sum_bar(unit, terms, FACTOR, st) + extra
            err = (got.double() - want).abs()
            r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
            worst["sums"] = max(worst["sums"], float(r.max()))
            if float(r.max()) > 1.0 or not torch.isfinite(r).all():
                fail("%s: %.3g x the bar; got %s want %s" % (name, float(r.max()), got.tolist(), want.tolist()))
    # 4. hidden layers
    for net_name in ("actor", "critic"):
        for l in (0, 2, 4):
            W = g["%s.%d.weight" % (net_name, l)]
            if W[B:].any() or W[:, B:].any():
                fail("%s.%d.weight gradient not zero outside its B x B block" % (net_name, l))


@pytest.mark.parametrize("clipped", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("path", list(PATHS))
def test_head_sample_by_sample(path, clipped, monkeypatch):
    precision, no_fused, fused, shadow, shapes_of = PATHS[path]
    if no_fused:
        monkeypatch.setenv("HGYM_NO_FUSED", "1")
    t0 = time.time()
    nets, fails, worst, jobs, seen = {}, [], dict(sample=0.0, sums=0.0, units=0.0), 0, set()
    for case in H.table():
        ref = H.reference(H.rows_of(case), case["mu"], case["v"], case["std"], unclipped=not clipped)
        un = H.units(ref)
        for shape in shapes_of(case):
            key = (shape, case["A"])
            if key not in nets:
                nets[key] = _net(shape, case["A"], precision)
                ld = (nets[key].shadow_ld(0), nets[key].shadow_ld(1))
                assert (ld[0] > 0 and ld[1] > 0) if fused else ld == (0, 0), (path, shape, ld)      # no row passes on another kernel
            tag = "%s %s %s %s" % (path, "clipped" if clipped else "unclipped", shape, case["name"])
            g, opt, same = _run(nets[key], case, shape, clipped, shadow)
            if not same:
                fails.append("%s: the second call left other bits" % tag)
            _check(tag, case, fused, precision == "bf16", g, opt, ref, un, fails, worst)
            jobs += 1
            seen.add((case["cls"], case["B"], case["A"]))
    # what the path must have reached
    As = {a for _, _, a in seen}
    Bs = {b for c, b, _ in seen if c == "bulk"}
    if path in ("f32", "bf16-generic"):
        assert As == set(H.A_ALL) and Bs >= set(H.B_XBOTL + H.B_G1)
    elif path == "fused-nopre":
        assert As == set(H.A_ALL) and Bs >= set(H.B_XBOTL + H.B_G1)
    else:
        assert As == {12} and Bs >= set(H.B_XBOTL)
    assert {c for c, _, _ in seen} == {"bulk", "vtie", "rbound", "ratio1"}
    what = "loss head %s, %s value loss, %d calls in %.1f s" % (path, "clipped" if clipped else "unclipped", jobs, time.time() - t0)
    print("\n%s: worst per-sample error %.3f x the bar, worst sum %.3f x the bar%s; K_REF %.3f, bar %.1f units%s" % (
        what, worst["sample"], worst["sums"], "" if precision == "bf16" else ", worst fp32 per-sample error %.3f units" % worst["units"],
        H.K_REF, FACTOR, " + 2^-8 |ref| (stored bf16)" if precision == "bf16" else ""))
    assert not fails, "%d failures, first ones:\n%s" % (len(fails), "\n".join(fails[:40]))
    BR.check(what + ": worst per-sample error / bar", worst["sample"], 1.0)
    BR.check(what + ": worst batch sum error / bar", worst["sums"], 1.0)
    if precision != "bf16":
        BR.check(what + ": worst per-sample error in units (K_REF %.3f)" % H.K_REF, worst["units"], FACTOR)
