"""CPU-only: the smoothness regulariser (hgym_ppo_grad_smooth, HgymSmooth) as far as it can be checked without a
device.

1. The float64 reference of tests/smoothness_common.py tells a wrong implementation from a right one: each of its switches (a gradient
   through the target, 1 / B for 1 / (B A), done rows not masked, successor r + 1 for r + N, the spatial target from the unperturbed row)
   moves at least one actor gradient tensor by at least SENSITIVITY x the path's bar, at the coefficients and the noise the GPU cases use.
2. The planted `dones` mask between a quarter and three quarters of the drawn rows, both kinds in every 64-row tile.
3. The successor map and the perturbation restated in numpy.
4. sizeof(HgymSmooth) against hgym_sizeof, the three symbols, make_smooth's refusals.
5. PPO.smoothness: parsing, defaults, the unknown-key and missing-noise_std errors, each refusal, the env's noise tiled over the frames,
   the train-config key."""
import ctypes as C

import numpy as np
import pytest
import torch

import smoothness_common as S
import update_options_common as U

O = U.Options
PATH_CASES = [O("bf16-fused", None, "scalar", False, False, False, False), O("f32-layer", None, "scalar", False, False, False, False),
              O("bf16-layer", U.TANH, "scalar", False, False, False, False), O("bf16-fused", U.TANH, "log", True, True, True, False)]


@pytest.mark.parametrize("opts", PATH_CASES, ids=[U.case_id(o) for o in PATH_CASES])
def test_every_wrong_variant_is_told_apart(opts):
    case = S.case_of(opts)
    S.check_mask(case)
    ref = S.reference(case)
    actor = [k for k in ref["grads"] if k.startswith("actor.")]
    bar = U.bar_of(opts)
    assert ref["smooth"][0] > 0 and ref["smooth"][1] > 0 and 0 < ref["smooth"][2] < case["B"]
    for wrong in S.WRONG:
        errs = U.errors(opts, S.reference(case, **wrong)["grads"], ref, names=actor)
        worst = max(errs.values())
        print("%s %s: worst actor tensor moves by %.3e = %.1f bars" % (U.case_id(opts), wrong, worst, worst / bar))
        assert worst >= U.SENSITIVITY * bar, (wrong, errs)
    # ... and each term alone against the plain update
    plain = U.reference(case["opts"], case["params"], case["stats"], case["cols"], case["idx"], case["ppo"])
    for lt, ls in ((S.LAM_T, 0.0), (0.0, S.LAM_S)):
        errs = U.errors(opts, S.reference(case, lam_t=lt, lam_s=ls)["grads"], plain, names=actor)
        assert max(errs.values()) >= U.SENSITIVITY * bar, (lt, ls, errs)
    off = S.reference(case, lam_t=0.0, lam_s=0.0)
    for k, g in plain["grads"].items():
        assert torch.equal(g, off["grads"][k]), k
    on = S.reference(case)
    for k, g in plain["grads"].items():      # nothing but the actor moves
        if not k.startswith("actor."):
            assert torch.equal(g, on["grads"][k]), k


def test_successor_map():
    T, N = 6, 4
    rng = np.random.default_rng(3)
    dones = (rng.random(T * N) < 0.4).astype(np.uint8)
    idx = rng.permutation(T * N)
    nxt, w = S.successor(idx, dones, N)
    assert nxt.dtype == np.int64 and w.dtype == np.float32
    for b, r in enumerate(idx):
        t, n = divmod(int(r), N)
        assert nxt[b] == (t + 1) * N + n      # the same env, one step later; t = T - 1 lands in slot T
        assert w[b] == (0.0 if dones[r] else 1.0)
    assert nxt.max() < (T + 1) * N and nxt.min() >= N


def test_perturbation_restated():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 9)).astype(np.float32)
    x[0, 0] = -0.0
    ns = np.linspace(0.0, 1.0, 9).astype(np.float32)
    rows = np.array([3, 0, 11, 5, 6, 2, 40])
    z = S.normals(S.SEED, 4, rows, 9)
    from oracle import philox as PH
    for m, r in enumerate(rows):      # the block of slot 128: normal c lives in Philox call 128 + c // 4
        assert np.array_equal(z[m], PH.normals(S.SEED, 4, np.uint32(r), 128, 9))
        assert np.array_equal(z[m, 4:8], PH.normals(S.SEED, 4, np.uint32(r), 129, 4))
    y = S.perturb(x, ns, S.SEED, 4, rows)
    assert np.array_equal(y[:, 0].view(np.uint32), x[:, 0].view(np.uint32))      # noise_std 0: the bits, -0.0 included
    assert np.allclose(y, x + ns * z, rtol=0, atol=1e-6) and not np.array_equal(y[:, 1:], x[:, 1:])
    assert not np.array_equal(S.normals(S.SEED, 5, rows, 9), z) and not np.array_equal(S.normals(S.SEED + 1, 4, rows, 9), z)


def test_struct_and_symbols():
    from hgym import _lib as L
    assert L.STRUCTS["HgymSmooth"] is L.Smooth and C.sizeof(L.Smooth) == L.lib.hgym_sizeof(b"HgymSmooth") == 72
    for name in ("hgym_smooth_pairs", "hgym_perturb_rows", "hgym_ppo_grad_smooth"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    assert L.SLOT_PERTURB == S.SLOT_PERTURB == 128


def test_make_smooth_refusals_and_defaults():
    import hgym
    s = hgym.make_smooth()
    assert s.temporal_coef == 0.0 and s.spatial_coef == 0.0 and not s.next_idx and not s.rows and not s.sums
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temporal_coef"):
            hgym.make_smooth(temporal_coef=bad)
        with pytest.raises(ValueError, match="spatial_coef"):
            hgym.make_smooth(spatial_coef=bad)
    assert hgym.smooth_ld(705) == 708 and hgym.smooth_ld(47) == 48 and hgym.smooth_ld(8) == 8
    # the library refuses before it looks at a device: no net is needed for these
    from hgym import _lib as L
    rc = L.lib.hgym_ppo_grad_smooth(None, None, None, None, None, None)
    assert rc == -1 and b"hgym_ppo_grad_smooth" in L.lib.hgym_last_error()
    assert L.lib.hgym_smooth_pairs(0, 4, None, None, None, None, None) == -1
    assert L.lib.hgym_perturb_rows(4, 5, None, 5, None, None, 0, None, None, 8, None) == -1


# ---------------------------------------------------------------------------------------------- PPO.smoothness, without a device
def test_ppo_smoothness_parsing_defaults_and_errors():
    from humanoid.algo.ppo import smoothness as SM
    assert SM.DEFAULTS == dict(temporal_coef=0.0, spatial_coef=0.0, noise_std=None, noise_scale=1.0, seed=None)
    assert SM.parse_config(None, 47) is None and SM.parse_config({}, 47) is None      # None, or both coefficients 0: off
    assert SM.parse_config(dict(temporal_coef=0.0, spatial_coef=0.0, noise_std=0.1), 47) is None
    c = SM.parse_config(dict(temporal_coef=2.0), 47, default_seed=99)
    assert c == dict(temporal_coef=2.0, spatial_coef=0.0, noise_std=None, seed=99)      # the run's seed by default; no noise needed
    c = SM.parse_config(dict(spatial_coef=1.5, noise_std=0.25, noise_scale=2.0, seed=7), 5)
    assert c["noise_std"] == [0.5] * 5 and c["seed"] == 7 and c["temporal_coef"] == 0.0      # a scalar fills the vector; noise_scale multiplies
    c = SM.parse_config(dict(spatial_coef=1.0, noise_std=np.arange(5, dtype=np.float32)), 5)
    assert c["noise_std"] == [0.0, 1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError, match="unknown key temporal"):
        SM.parse_config(dict(temporal=1.0), 5)
    with pytest.raises(ValueError, match="needs noise_std"):
        SM.parse_config(dict(spatial_coef=1.0), 5)
    with pytest.raises(ValueError, match="has 4 values"):
        SM.parse_config(dict(spatial_coef=1.0, noise_std=[0.1] * 4), 5)
    for k in ("temporal_coef", "spatial_coef", "noise_scale"):
        for bad in (-1.0, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match=k):
                SM.parse_config({"temporal_coef": 1.0, k: bad}, 5)
    with pytest.raises(ValueError, match="noise_std"):
        SM.parse_config(dict(spatial_coef=1.0, noise_std=[-0.1] * 5), 5)
    with pytest.raises(ValueError, match="a dict"):
        SM.parse_config(3.0, 5)


def test_ppo_smoothness_refusals_need_no_device():
    from humanoid.algo.ppo import smoothness as SM
    SM.check_setup()
    with pytest.raises(ValueError, match="one rank"):
        SM.check_setup(world=2)
    with pytest.raises(ValueError, match="symmetry"):
        SM.check_setup(symmetry=object())
    with pytest.raises(ValueError, match="Distillation"):
        SM.check_setup(distillation=True)


def test_env_noise_std_is_tiled_over_the_frames():
    from types import SimpleNamespace
    from humanoid.algo.ppo import smoothness as SM
    cfg = SimpleNamespace(noise=SimpleNamespace(noise_level=0.5))
    assert SM.env_noise_std(cfg, [0.0, 2.0, 4.0], 6) == [0.0, 1.0, 2.0, 0.0, 1.0, 2.0]
    assert SM.env_noise_std(cfg, None, 6) is None and SM.env_noise_std(cfg, [1.0, 2.0, 3.0, 4.0], 6) is None
    assert SM.env_noise_std(SimpleNamespace(), [1.0], 3) is None


def test_train_config_key_is_not_a_ppo_argument():
    from humanoid.algo.ppo import on_policy_runner as R
    kw, sym = R._split_algorithm_cfg(dict(clip_param=0.2, smoothness_cfg=dict(temporal_coef=1.0)))
    assert kw == dict(clip_param=0.2) and sym is False and R.SMOOTH_KEY == "smoothness_cfg"
    from humanoid.envs import XBotLCfgPPO
    assert not hasattr(XBotLCfgPPO.algorithm, "smoothness_cfg")
