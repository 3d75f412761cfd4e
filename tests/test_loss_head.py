"""Host side of the per-sample loss-head tests (tests/loss_head_common.py has the probe, the float64 autograd reference, the case table
and the tolerances): the probe plants mu and V bit-exactly, oracle/ppo_oracle.py's hand-written backward agrees with float64 autograd on
every case (ties and boundaries included), and the table really holds what tests/test_loss_head_gpu.py relies on, so that a pass there
cannot be vacuous."""
import math

import numpy as np
import pytest
import torch

import loss_head_common as H
from oracle import ppo_oracle as P

CASES = H.table()
IDS = [c["name"] for c in CASES]
F64_TOL = 1e-12          # float64 against float64, relative to the largest entry


def _ref(case, unclipped=False):
    return H.reference(H.rows_of(case), case["mu"], case["v"], case["std"], unclipped=unclipped)


def _bound_distance(ref):
    lr = ref["log_ratio"]
    return torch.minimum((lr - math.log1p(H.PPO["clip"])).abs(), (lr - math.log1p(-H.PPO["clip"])).abs())


def test_table_covers_the_batch_sizes_action_counts_and_bands():
    bulk = [c for c in CASES if c["cls"] == "bulk"]
    assert {c["B"] for c in bulk if c["A"] == 12} == set(H.B_XBOTL + H.B_G1)
    assert {c["A"] for c in bulk} == set(H.A_ALL)
    assert {c["band"] for c in bulk if c["A"] == 12} == set(H.BANDS) == {c["band"] for c in bulk if c["A"] != 12}
    assert {c["cls"] for c in CASES} == {"bulk", "vtie", "rbound", "ratio1"}
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_storage_is_nan_outside_the_scattered_index_list(case):
    B, S, idx = case["B"], case["S"], case["idx"]
    assert S > B and idx.shape == (B,) and len(set(idx.tolist())) == B and int(idx.max()) < S
    if B > 1:
        assert not torch.equal(idx, torch.arange(B)) and not torch.equal(idx, idx.sort().values)      # neither a prefix nor ordered
    rest = torch.ones(S, dtype=torch.bool)
    rest[idx] = False
    assert int(rest.sum()) == S - B >= 7
    for k, t in case["cols"].items():
        assert t.dtype == torch.float32 and t.shape[0] == S
        assert torch.isnan(t[rest]).all(), k
        assert torch.isfinite(t[idx]).all(), k
    n_obs, n_priv = 40, 300
    obs, priv = H.storage_inputs(case, n_obs, n_priv, torch.zeros(B, n_obs), torch.zeros(B, n_priv))
    assert torch.isnan(obs[rest]).all() and torch.isnan(priv[rest]).all() and not torch.isnan(obs[idx]).any()
    band = H.BANDS[case["band"]]
    assert float(case["std"].min()) >= band[0] and float(case["std"].max()) <= band[1]
    so = case["cols"]["sigma_old"][idx]
    assert float(so.min()) >= band[0] and float(so.max()) <= band[1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probe_plants_mu_and_v_bit_exactly(case):
    """Through P.mlp_forward at every network shape the case runs on, plain and with bf16 operands; and the head weight gradient of the
    oracle is the per-sample head gradient, bit for bit."""
    shapes = H.shapes_for(case)
    assert shapes
    for shape in shapes:
        n_obs, n_priv, ah, ch = H.SHAPES[shape]
        p, obs, priv = H.probe_params(n_obs, n_priv, case["A"], ah, ch, case["mu"], case["v"], case["std"])
        for quant in (None, P.bf16_round):
            assert torch.equal(P.mlp_forward(obs, p.actor, quant=quant), case["mu"]), (shape, quant)
            assert torch.equal(P.mlp_forward(priv, p.critic, quant=quant).squeeze(-1), case["v"]), (shape, quant)
    out = H.run_oracle(case, torch.float32)
    B = case["B"]
    assert torch.equal(out["mu"], case["mu"]) and torch.equal(out["val"], case["v"])
    Wa, ba = out["grads"].actor[-1]
    Wc, bc = out["grads"].critic[-1]
    assert torch.equal(Wa[:, :B].t(), out["d_mu"]) and not Wa[:, B:].any()
    assert torch.equal(Wc[0, :B], out["d_val"]) and not Wc[:, B:].any()
    for W, _ in out["grads"].actor[:-1] + out["grads"].critic[:-1]:
        assert not W[B:].any() and not W[:, B:].any() and torch.isfinite(W).all()


def _close(got, want, scale=None):
    scale = float(want.abs().max()) if scale is None else float(scale)
    err = float((got.double() - want).abs().max())
    return err <= F64_TOL * scale, (err, scale)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_hand_backward_against_float64_autograd(case):
    """P.ppo_loss_and_grads in float64 against torch.autograd of the plainly written loss: per-sample d_mu and d_val, d_std and the four
    scalars, at 1e-12 of the largest entry."""
    ref = _ref(case)
    out = H.run_oracle(case, torch.float64)
    B = case["B"]
    for got, want in ((out["d_mu"], ref["g_mu"]), (out["d_val"], ref["d_v"])):
        ok, info = _close(got, want)
        assert ok, info
    ok, info = _close(out["grads"].std, ref["g_sigma"].sum(0), ref["g_sigma"].abs().sum(0).max())
    assert ok, info
    for key, per_sample, scale in (("surrogate", ref["surr"], ref["surr"].abs()), ("value_loss", ref["vl"], ref["vl"].abs()),
                                   ("entropy", ref["ent"], ref["t_ent"]), ("kl", ref["kl"], ref["t_kl"])):
        ok, info = _close(out[key] * B, per_sample.sum(), scale.sum())
        assert ok, (key, info)
    # the head bias gradients are the sums the GPU test reads
    ok, info = _close(out["grads"].actor[-1][1], ref["g_mu"].sum(0), ref["g_mu"].abs().sum(0).max())
    assert ok, info


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unclipped_reference_against_its_closed_form(case):
    """The oracle has the clipped value loss only: the autograd reference of (R - V)^2.mean() against 2 coef (V - R) / B."""
    ref, rows = _ref(case, unclipped=True), H.rows_of(case)
    want = 2.0 * H.PPO["value_coef"] * (case["v"].double() - rows["returns"].double()) / case["B"]
    ok, info = _close(ref["d_v"], want)
    assert ok, info
    assert torch.equal(ref["g_mu"], _ref(case)["g_mu"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_strict_samples_keep_their_margin_and_fp32_takes_the_float64_side(case):
    ref = _ref(case)
    dist = _bound_distance(ref)
    out32 = H.run_oracle(case, torch.float32)
    lpo = H.rows_of(case)["logp"]
    ratio32 = torch.exp(out32["logp"] - lpo)
    clip32 = torch.tensor(H.PPO["clip"], dtype=torch.float32)
    in32 = (ratio32 >= 1.0 - clip32) & (ratio32 <= 1.0 + clip32)
    ratio64 = torch.exp(ref["log_ratio"])
    in64 = (ratio64 >= 1.0 - H.PPO["clip"]) & (ratio64 <= 1.0 + H.PPO["clip"])
    assert float(ref["log_ratio"].abs().max()) <= H.MAX_LOG_RATIO
    if case["cls"] == "rbound":          # boundary-class samples: cases of their own, and really on the bound
        ulp = torch.from_numpy(np.spacing(np.abs(lpo.numpy()))).double()      # lp_old: the fp32 nearest the bound and its 1, 2, 4 ulp neighbours
        assert case["boundary"].all() and (dist <= 4.5 * ulp).all()
        return
    assert not case["boundary"].any()
    assert float(dist.min()) >= H.STRICT_MARGIN, float(dist.min())
    assert torch.equal(in32, in64)
    near = [i for i, k in enumerate(case["kinds"]) if "near" in k]
    if near:
        assert float(dist[near].max()) <= 2e-3
    if case["cls"] == "ratio1":          # the s1 == s2 tie every in-range sample takes, with a gradient to show it
        assert in64.all() and float(ref["log_ratio"].abs().max()) <= 1e-4 and (H.rows_of(case)["adv"] != 0).all()


def test_fp32_ratio_straddles_the_bound_in_the_boundary_cases():
    seen = set()
    for case in CASES:
        if case["cls"] != "rbound":
            continue
        out32 = H.run_oracle(case, torch.float32)
        rows = H.rows_of(case)
        ratio32 = torch.exp(out32["logp"] - rows["logp"])
        clip32 = torch.tensor(H.PPO["clip"], dtype=torch.float32)
        for i, kind in enumerate(case["kinds"]):
            inside = bool(ratio32[i] <= 1.0 + clip32) if kind == "hi_bound" else bool(ratio32[i] >= 1.0 - clip32)
            seen.add((kind, inside))
        # the sign of the advantage makes the indicator decide: the two float64 variants differ by the whole gradient
        ref = _ref(case)
        assert float((ref["g_mu_in"] - ref["g_mu_out"]).abs().amax(-1).min()) > 0 and not ref["g_mu_out"].any()
    assert seen == {("hi_bound", True), ("hi_bound", False), ("lo_bound", True), ("lo_bound", False)}, seen


def test_value_ties_are_exact_in_float32_and_float64():
    edge, mid = H.value_tie_pairs()
    assert len(edge) >= 8 and len(mid) >= 4, (len(edge), len(mid))
    c32 = H.CLIP32
    for case in (c for c in CASES if c["cls"] == "vtie"):
        rows = H.rows_of(case)
        v, vold, ret = case["v"].numpy(), rows["values"].numpy(), rows["returns"].numpy()
        assert v.dtype == np.float32 and case["B"] == 2 * len(edge) + len(mid)
        n_edge = n_mid = 0
        sides = set()
        for i in range(case["B"]):
            d = np.float32(v[i] - vold[i])
            vc = np.float32(vold[i] + np.clip(d, -c32, c32))
            l1, l2 = np.float32(v[i] - ret[i]) ** 2, np.float32(vc - ret[i]) ** 2
            d64 = float(v[i]) - float(vold[i])
            vc64 = float(vold[i]) + min(max(d64, -float(c32)), float(c32))
            assert l1 == l2 and (float(v[i]) - float(ret[i])) ** 2 == (vc64 - float(ret[i])) ** 2      # every row is an exact l1 == l2 tie
            if abs(d) == c32:
                assert abs(d64) == float(c32)
                n_edge += 1
                sides.add((float(d) > 0, bool(ret[i] > v[i])))
            else:
                assert abs(d64) > float(c32) and l1 > 0
                n_mid += 1
        assert (n_edge, n_mid) == (2 * len(edge), len(mid)) and len(sides) == 4      # +-clip, returns on both sides
        # the tie weight is visible: autograd's half gradient on the midpoint rows, the full one on the +-clip rows
        ref = _ref(case)
        full = 2.0 * H.PPO["value_coef"] * (case["v"].double() - rows["returns"].double()) / case["B"]
        is_edge = torch.from_numpy(np.abs((v - vold).astype(np.float32)) == c32)
        assert torch.allclose(ref["d_v"], torch.where(is_edge, full, 0.5 * full), rtol=1e-14, atol=0)


def test_bulk_cases_hold_every_class():
    singles = [c for c in CASES if c["cls"] == "bulk" and c["B"] == 1]
    for case in (c for c in CASES if c["cls"] == "bulk"):
        ref, rows = _ref(case), H.rows_of(case)
        ratio = torch.exp(ref["log_ratio"])
        hi, lo = ratio > 1.0 + H.PPO["clip"], ratio < 1.0 - H.PPO["clip"]
        B = case["B"]
        if B == 1:
            continue
        assert B >= 15
        assert int(hi.sum()) >= 0.2 * B and int(lo.sum()) >= 0.2 * B and int((~hi & ~lo).sum()) >= 0.2 * B, case["name"]
        assert int((rows["adv"] == 0).sum()) >= 3
        mag = rows["adv"].abs()[rows["adv"] != 0]
        assert (rows["adv"] > 0).any() and (rows["adv"] < 0).any() and float(mag.min()) >= 1e-3 and float(mag.max()) <= 1e2
        dv = (case["v"] - rows["values"]).abs()
        assert (dv > 0.2 + 5e-3).any() and (dv < 0.2 - 5e-3).any() and not ((dv - 0.2).abs() < 5e-3).any()
        assert {k for k in case["kinds"] if "near" in k} == {"hi_near_out", "lo_near_out", "hi_near_in", "lo_near_in"}
    # one sample cannot hold every class: the single-sample cases do together
    assert {c["kinds"][0] for c in singles} >= {"in", "hi_far", "lo_near_out", "hi_near_in"}
    assert any(float(H.rows_of(c)["adv"][0]) == 0 for c in singles)


def test_k_ref():
    """K_REF: the worst error of the oracle evaluated in fp32 on the CPU, in units, over every per-sample g_mu and d_v of the table; and
    the sums of the same run hold the sum bars the GPU paths are given (the formula is sound before it meets a kernel)."""
    worst, where = 0.0, None
    for case in CASES:
        ref = _ref(case)
        un = H.units(ref)
        out = H.run_oracle(case, torch.float32)
        k = max(float(H.mu_excess(out["d_mu"], ref, un, case["boundary"], 1.0).max()),
                float(H.excess(out["d_val"], ref["d_v"], un["d_v"], 1.0).max()))
        if k > worst:
            worst, where = k, case["name"]
        if case["cls"] == "rbound":
            continue
        B = case["B"]
        for got, terms, unit in ((out["grads"].std, ref["g_sigma"], un["g_sigma"]), (out["grads"].actor[-1][1], ref["g_mu"], un["g_mu"]),
                                 (out["surrogate"] * B, ref["surr"], un["surr"]), (out["value_loss"] * B, ref["vl"], un["vl"]),
                                 (out["entropy"] * B, ref["ent"], un["ent"]), (out["kl"] * B, ref["kl"], un["kl"])):
            err = (got.double() - terms.sum(0)).abs()
            # (+ one fp32 rounding of the mean the oracle returns)
            bar = H.sum_bar(unit, terms, H.GPU_FACTOR * H.K_REF) + H.U24 * terms.sum(0).abs()
            assert (err <= bar).all(), (case["name"], err, bar)
    print("\nK_ref measured %.3f (worst case %s); module value %.3f, GPU bar %.1f units" % (worst, where, H.K_REF, H.GPU_FACTOR * H.K_REF))
    assert abs(worst - H.K_REF) <= 0.25 * H.K_REF, (worst, H.K_REF)
