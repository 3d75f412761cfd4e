"""CPU-only: the mirror loss and the smoothness regulariser in one actor head (hgym_ppo_grad_smooth_mirror, PPO.mirror_loss_coef beside
PPO.smoothness) as far as it can be checked without a device.

1. tests/mirror_smooth_common.py's float64 reference against torch autograd run end to end in float64 through the whole net (the f32 path:
   no operand rounding), every target detached by hand there; and every deliberately wrong variant -- a term left out, the action table
   not applied, w ignored, a target not detached -- moves some actor tensor by at least SENSITIVITY x the path's bar.
2. The reference is the sum of its parts: its d mu is the plain head's plus each single-term reference's increment, nothing but the actor
   moves, and with two terms at 0 it is the single-option reference.
3. PPO.check_setup: the mirror loss without augmentation beside the regulariser passes; augmentation beside it, two ranks and Distillation
   still raise.
4. The noise-invariance check names the column; the env's own noise vector passes.
5. The new symbol through ctypes: the prototype, and the refusals that need no device."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import mirror_loss_common as M
import mirror_smooth_common as MS
import smoothness_common as S
import update_options_common as U
from oracle import ppo_oracle as P

O = U.Options
PATH_CASES = [O("bf16-fused", None, "scalar", False, False, False, False), O("f32-layer", None, "scalar", False, False, False, False),
              O("bf16-layer", U.TANH, "scalar", False, False, False, False), O("bf16-fused", U.TANH, "log", True, True, True, False)]


def _autograd(case, coef, lam_t, lam_s):
    """The loss of the definition, written once in torch float64 over leaf copies of the parameters; the three targets under no_grad."""
    opts, cols, idx = case["opts"], case["cols"], case["idx"]
    assert opts.path == "f32-layer" and not opts.norm and not opts.aux and opts.activation is None and opts.std == "scalar"
    p = {k: v.double().clone().requires_grad_() for k, v in case["params"].items()}

    def mlp(x, net):
        l = 0
        while "%s.%d.weight" % (net, 2 * l) in p:
            x = F.linear(x, p["%s.%d.weight" % (net, 2 * l)], p["%s.%d.bias" % (net, 2 * l)])
            l += 1
            if "%s.%d.weight" % (net, 2 * l) in p:
                x = F.elu(x)
        return x
    obs = cols[0].double()
    act, vold, adv, ret, lpo, mo, so = (t[idx].double() for t in cols[2:])
    mu, v = mlp(obs[idx], "actor"), mlp(cols[1][idx].double(), "critic").squeeze(-1)
    B, A = mu.shape
    with torch.no_grad():
        src, sign = torch.tensor(case["spec"].act_src), torch.tensor(case["spec"].act_sign, dtype=torch.float64)
        tm = sign * mlp(obs[case["pair"]], "actor")[:, src]
        tT = mlp(obs[case["nxt"]], "actor")
        tS = mlp(S.clean_near(case).double(), "actor")
    sig = p["std"].expand(B, A)
    ppo = case["ppo"]
    ratio = torch.exp(P.gaussian_log_prob(act, mu, sig) - lpo)
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - ppo["clip"], 1.0 + ppo["clip"]))
    vc = vold + (v - vold).clamp(-ppo["clip"], ppo["clip"])
    vl = (ret - v).pow(2) if opts.unclipped else torch.max((v - ret).pow(2), (vc - ret).pow(2))
    loss = surr.mean() + ppo["value_coef"] * vl.mean() - ppo["entropy_coef"] * P.gaussian_entropy(sig).mean()
    w = case["weight"].double()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    loss = loss + f32(coef) / (B * A) * ((mu - tm) ** 2).sum() + f32(lam_t) / (B * A) * (w[:, None] * (mu - tT) ** 2).sum() \
        + f32(lam_s) / (B * A) * ((mu - tS) ** 2).sum()
    names = list(p)
    return dict(zip(names, torch.autograd.grad(loss, [p[k] for k in names])))


@pytest.mark.parametrize("lams", [(MS.COEF, MS.LAM_T, MS.LAM_S), (MS.COEF, 0.0, MS.LAM_S), (0.25, MS.LAM_T, 0.0)])
def test_reference_against_autograd(lams):
    opts = PATH_CASES[1]
    case = MS.case_of(opts)
    ref = MS.reference(case, coef=lams[0], lam_t=lams[1], lam_s=lams[2])
    auto = _autograd(case, *lams)
    for k, g in ref["grads"].items():
        err = float((g - auto[k]).abs().max() / auto[k].abs().max())
        print("%-18s %.3e" % (k, err))
        assert err <= 1e-11, k      # two float64 evaluations of one expression, summed in different orders


@pytest.mark.parametrize("opts", PATH_CASES, ids=[U.case_id(o) for o in PATH_CASES])
def test_every_wrong_variant_is_told_apart(opts):
    case = MS.case_of(opts)
    S.check_mask(case)
    ref = MS.reference(case)
    actor = [k for k in ref["grads"] if k.startswith("actor.")]
    bar = U.bar_of(opts)
    assert ref["mirror"] > 0 and ref["smooth"][0] > 0 and ref["smooth"][1] > 0 and 0 < ref["smooth"][2] < case["B"]
    for wrong in MS.WRONG:
        errs = U.errors(opts, MS.reference(case, **wrong)["grads"], ref, names=actor)
        worst = max(errs.values())
        print("%s %s: worst actor tensor moves by %.3e = %.1f bars" % (U.case_id(opts), wrong, worst, worst / bar))
        assert worst >= U.SENSITIVITY * bar, (wrong, errs)


@pytest.mark.parametrize("opts", PATH_CASES[:2], ids=[U.case_id(o) for o in PATH_CASES[:2]])
def test_reference_is_the_sum_of_its_parts(opts):
    case = MS.case_of(opts)
    ref = MS.reference(case)
    plain = U.reference(case["opts"], case["params"], case["stats"], case["cols"], case["idx"], case["ppo"])
    mirror = M.reference(case, coef=MS.COEF)
    smooth = S.reference(case)
    for k, g in plain["grads"].items():      # nothing but the actor moves
        if not k.startswith("actor."):
            assert torch.equal(g, ref["grads"][k]), k
    inc = (mirror["d_mu"] - plain["d_mu"]) + (smooth["d_mu"] - plain["d_mu"])
    assert float((ref["d_mu"] - plain["d_mu"] - inc).abs().max()) <= 1e-12 * float(ref["d_mu"].abs().max())
    assert abs(ref["mirror"] - mirror["mirror"]) <= 1e-12 * mirror["mirror"]
    assert all(abs(a - b) <= 1e-12 * max(b, 1e-300) for a, b in zip(ref["smooth"], smooth["smooth"]))
    # two terms at 0: the single-option references themselves
    only_m = MS.reference(case, lam_t=0.0, lam_s=0.0)
    only_s = MS.reference(case, coef=0.0)
    for k in ref["grads"]:
        assert torch.equal(only_m["grads"][k], mirror["grads"][k]), k
        # (the two smoothness increments join d mu one after the other here, as one sum there: the last bits may differ)
        assert float((only_s["grads"][k] - smooth["grads"][k]).abs().max()) <= 1e-12 * float(smooth["grads"][k].abs().max()), k


# ---------------------------------------------------------------------------------------------- PPO, without a device
def test_check_setup_lets_the_mirror_loss_without_augmentation_through():
    from humanoid.algo import PPO
    spec = U.xbot_l_spec()
    sm = dict(temporal_coef=1.0, spatial_coef=1.0, noise_std=0.1)
    kw = dict(num_envs=8, num_transitions_per_env=4, num_mini_batches=2, num_actor_obs=705)
    PPO.check_setup(**kw, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=0.5, smoothness=sm)      # (today: ValueError)
    PPO.check_setup(**kw, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=0.5, smoothness=dict(temporal_coef=2.0))
    with pytest.raises(ValueError, match="symmetry"):      # augmentation: the mirrored half has no bootstrap slot
        PPO.check_setup(**kw, symmetry=spec, symmetry_augmentation=True, mirror_loss_coef=0.5, smoothness=sm)
    with pytest.raises(ValueError, match="symmetry"):
        PPO.check_setup(**kw, symmetry=spec, symmetry_augmentation=True, smoothness=sm)
    with pytest.raises(ValueError, match="one rank"):
        PPO.check_setup(**kw, world=2, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=0.5, smoothness=sm)
    with pytest.raises(ValueError, match="needs the mirror tables"):
        PPO.check_setup(**kw, mirror_loss_coef=0.5, smoothness=sm)
    PPO.check_setup(**kw, symmetry=spec, symmetry_augmentation=False, mirror_loss_coef=0.5)      # either alone, as before
    PPO.check_setup(**kw, smoothness=sm)


def test_distillation_still_refuses_the_regulariser():
    from humanoid.algo.ppo import smoothness as SM
    with pytest.raises(ValueError, match="Distillation"):
        SM.check_setup(1, None, True)
    with pytest.raises(ValueError, match="symmetry"):      # the module's own refusal is not lifted
        SM.check_setup(symmetry=object())


def _env_noise():
    """The env's per-column noise as LeggedRobot builds it from the XBot-L config, times noise_level, tiled over the 15 frames."""
    from types import SimpleNamespace
    from humanoid.algo.ppo import smoothness as SM
    from humanoid.envs import XBotLCfg
    ns_, os_ = XBotLCfg.noise.noise_scales, XBotLCfg.normalization.obs_scales
    vec = [0.0] * 5 + [ns_.dof_pos * os_.dof_pos] * 12 + [ns_.dof_vel * os_.dof_vel] * 12 + [0.0] * 12 + [ns_.ang_vel * os_.ang_vel] * 3 + \
          [ns_.quat * os_.quat] * 3
    return SM.env_noise_std(SimpleNamespace(noise=SimpleNamespace(noise_level=XBotLCfg.noise.noise_level)), vec, 705)


def test_noise_must_be_invariant_under_the_mirror_table():
    from humanoid.algo.ppo import smoothness as SM
    spec = U.xbot_l_spec()
    ns = _env_noise()
    assert len(ns) == 705 and max(ns) > 0
    SM.check_noise_mirror(ns, spec.obs_src)      # the env's own vector passes
    SM.check_noise_mirror(torch.tensor(ns), torch.tensor(spec.obs_src))
    SM.check_noise_mirror([0.3] * 705, spec.obs_src)
    bad = list(ns)
    c = 47 * 3 + 5 + 2      # frame 3, joint position 2 (a left-leg joint): its mirror column is joint 8 of the same frame
    assert spec.obs_src[c] == 47 * 3 + 5 + 8
    bad[c] = bad[c] + 0.5
    with pytest.raises(ValueError, match=r"column %d has .* mirror column %d" % (c, spec.obs_src[c])):
        SM.check_noise_mirror(bad, spec.obs_src)
    bad2 = list(bad)
    bad2[7] += 1.0      # the FIRST column that breaks it is named
    with pytest.raises(ValueError, match=r"column 7 has"):
        SM.check_noise_mirror(bad2, spec.obs_src)
    with pytest.raises(ValueError, match="704 values"):
        SM.check_noise_mirror(ns[:-1], spec.obs_src)


def test_smoothness_object_owns_head_partials_only_beside_the_mirror_loss():
    import hgym
    assert [hgym.smooth_mirror_partials(b) for b in (1, 63, 64, 65, 200, 61440)] == [4, 4, 4, 8, 16, 3840]
    from humanoid.algo.ppo import smoothness as SM
    cfg = SM.parse_config(dict(temporal_coef=1.0), 8)
    off = SM.Smoothness(cfg, 20, 10, 8, 3, "cpu")
    on = SM.Smoothness(cfg, 20, 130, 8, 3, "cpu", mirror_loss=True)
    assert off.head_partials is None and on.head_partials.numel() == 12 and on.head_partials.dtype == torch.float32
    assert len(off.graph_key()["smoothness"]) == 3 + len(SM.Smoothness.BUFFERS)      # unchanged while the mirror loss is off
    assert on.graph_key()["smoothness"][-1] == on.head_partials.data_ptr() and len(on.graph_key()["smoothness"]) == 4 + len(SM.Smoothness.BUFFERS)
    assert off.log_parts()[0][0] == on.log_parts()[0][0] == "smooth"


# ---------------------------------------------------------------------------------------------- the symbol, without a device
def test_symbol_and_refusals_that_need_no_device():
    from hgym import _lib as L
    name = "hgym_ppo_grad_smooth_mirror"
    assert name in L.SYMBOLS and hasattr(L.lib, name)
    assert len(L.SYMBOLS[name][1]) == 8 and L.SYMBOLS[name][1][-2] is C.c_int64
    f = L.lib.hgym_ppo_grad_smooth_mirror
    assert f(None, None, None, None, None, None, 0, None) == -1 and name.encode() in L.lib.hgym_last_error()
    cfg, ppo, net, batch, sm = L.NetConfig(), L.PPOConfig(), L.Net(), L.Batch(), L.Smooth()
    ref = lambda *xs: [C.byref(x) for x in xs]
    for bad in (-1.0, float("nan"), float("inf")):
        sm.temporal_coef, sm.spatial_coef = bad, 0.0
        assert f(*ref(cfg, ppo, net, batch, sm), None, 0, None) == -1 and b"temporal_coef" in L.lib.hgym_last_error()
    sm.temporal_coef, sm.spatial_coef = 1.0, 0.0
    ppo.world_size = 2
    assert f(*ref(cfg, ppo, net, batch, sm), None, 0, None) == -1 and b"world_size" in L.lib.hgym_last_error()
    ppo.world_size = 1
    assert f(*ref(cfg, ppo, net, batch, sm), None, 0, None) == -1 and b"sums" in L.lib.hgym_last_error()
    # all terms on: head_partials is looked at before any net -- NULL, misaligned, too short
    sums = (C.c_double * 4)()
    w, tn = (C.c_float * 200)(), (C.c_float * 2400 * 2)()
    nxt = (C.c_int64 * 200)()
    sm.sums = C.cast(sums, L.c_f64_p)
    sm.next_idx, sm.next_weight = C.cast(nxt, L.c_i64_p), C.cast(w, L.c_float_p)
    sm.target_next = C.cast((C.addressof(tn) + 15) // 16 * 16, L.c_float_p)
    ppo.mirror_coef = 0.5
    batch.B = 65
    hp = (C.c_float * 64)()
    base = (C.addressof(hp) + 15) // 16 * 16
    assert f(*ref(cfg, ppo, net, batch, sm), None, 8, None) == -1 and b"head_partials" in L.lib.hgym_last_error()
    assert f(*ref(cfg, ppo, net, batch, sm), C.cast(base + 4, L.c_float_p), 8, None) == -1 and b"16-byte" in L.lib.hgym_last_error()
    assert f(*ref(cfg, ppo, net, batch, sm), C.cast(base, L.c_float_p), 7, None) == -1 and b"needs 8 floats" in L.lib.hgym_last_error()
    assert sums[3] == 0.0
