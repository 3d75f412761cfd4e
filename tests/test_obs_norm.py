"""CPU-only: the host side of empirical observation normalisation -- the block's layout query, the struct mirrors,
the constructor / train-config plumbing, and the float64 restatement of the merge (tests/obs_norm_common.py) on a hand-computed example.
The device side is tests/test_obs_norm_gpu.py and tests/test_obs_norm_runner_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import obs_norm_common as ON


def _cfg(precision, aux=False, num_obs=705, num_priv=219):
    from hgym import make_net_config
    kw = dict(aux_hidden=[512, 256, 256], aux_out=73, aux_target_offset=num_priv - 73) if aux else {}
    return make_net_config(num_obs, num_priv, 12, [512, 256, 128], [768, 256, 128], precision, 4096, **kw)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("aux", [False, True])
def test_layout_is_aligned_and_parts_do_not_overlap(precision, aux):
    from hgym import norm_layout, _lib as L
    cfg = _cfg(precision, aux)
    lay = norm_layout(cfg)
    assert len(lay) == L.NORM_LAYOUT
    K, N1 = (705, 219), (512, 768, 512)
    wgs = [lay[L.NORM_WGS + k] for k in (0, 1)]
    assert all(w >= 1 for w in wgs) and lay[L.NORM_ROWS_PER_WG] >= 4 and lay[L.NORM_ROWS_PER_WG] % 4 == 0
    assert lay[L.NORM_SUMS_DOUBLES] == 2 + 2 * (K[0] + K[1])
    parts = [(lay[L.NORM_HEADER], L.NORM_HEADER_DOUBLES * 8), (lay[L.NORM_SUMS], lay[L.NORM_SUMS_DOUBLES] * 8)]
    for k in (0, 1):
        parts += [(lay[L.NORM_MEAN + k], K[k] * 8), (lay[L.NORM_VAR + k], K[k] * 8), (lay[L.NORM_MEAN_F + k], K[k] * 4),
                  (lay[L.NORM_SCALE_F + k], K[k] * 4), (lay[L.NORM_PARTIALS + k], wgs[k] * 2 * K[k] * 8)]
    for i in range(3 if aux else 2):
        parts.append((lay[L.NORM_BIAS + i], N1[i] * 4))
    if not aux:
        assert lay[L.NORM_BIAS + 2] == -1
    parts.sort()
    for off, size in parts:
        assert off >= 0 and off % 256 == 0 and size > 0
    for (o0, s0), (o1, _) in zip(parts, parts[1:]):
        assert o0 + s0 <= o1, "parts overlap"
    assert parts[-1][0] + parts[-1][1] <= lay[L.NORM_BYTES] and lay[L.NORM_BYTES] % 256 == 0


def test_layout_refuses_a_bad_config():
    from hgym import _lib as L
    out = (C.c_int64 * L.NORM_LAYOUT)()
    cfg = _cfg("f32")
    cfg.actor_dims[0] = 700                 # inconsistent with num_obs
    assert L.lib.hgym_net_norm_layout(C.byref(cfg), out) == -2 and b"inconsistent" in L.lib.hgym_last_error()
    assert L.lib.hgym_net_norm_layout(None, out) == -1
    wide = _cfg("f32", num_obs=1025)        # beyond what the accumulate kernel's LDS takes
    assert L.lib.hgym_net_norm_layout(C.byref(wide), out) == -4 and b"1024" in L.lib.hgym_last_error()
    # the entry points that need the block refuse a net without one, before anything is launched
    net = L.Net()
    assert L.lib.hgym_net_norm_merge(C.byref(_cfg("f32")), C.byref(net), None) == -1 and b"norm" in L.lib.hgym_last_error()


def test_struct_mirror_has_norm_as_the_last_member_of_net():
    from hgym import _lib as L
    assert L.Net._fields_[-1][0] == "norm" and [f[0] for f in L.Net._fields_[:6]] == ["params", "grads", "adam_m", "adam_v", "opt_state", "workspace"]
    assert C.sizeof(L.Net) == L.lib.hgym_sizeof(b"HgymNet") == 7 * 8
    assert L.Net.norm.offset == 6 * 8
    assert L.Net().norm is None                                   # a default-constructed net: off
    assert L.Net(None, None, None, None, None, None).norm is None       # the positional construction of before
    for name, st in L.STRUCTS.items():
        assert C.sizeof(st) == L.lib.hgym_sizeof(name.encode()), name
    assert [f[0] for f in L.NetConfig._fields_[-2:]] == ["std_param", "fused_activation"]      # HgymNetConfig gained nothing
    assert L.lib.hgym_version() == 9
    for sym in ("hgym_net_norm_layout", "hgym_net_norm_init", "hgym_net_norm_accumulate", "hgym_net_norm_merge", "hgym_net_norm_unfold_grad"):
        assert sym in L.SYMBOLS and hasattr(L.lib, sym)


def test_actor_critic_constructor():
    import torch.nn as nn
    from humanoid.algo import ActorCritic
    from humanoid.algo.ppo.normalizer import EmpiricalNormalization
    off = ActorCritic(37, 19, 5, [24, 16], [24, 16])
    assert off.empirical_normalization is False and off.obs_norm_spec is None
    assert isinstance(off.obs_normalizer, nn.Identity) and isinstance(off.critic_obs_normalizer, nn.Identity) and off.norm_state_dicts() == {}
    on = ActorCritic(37, 19, 5, [24, 16], [24, 16], empirical_normalization=True)
    assert on.obs_norm_spec == (1e-2, None)
    assert isinstance(on.obs_normalizer, EmpiricalNormalization) and on.obs_normalizer.num_columns == 37
    assert on.critic_obs_normalizer.num_columns == 19 and on.critic_obs_normalizer.which == 1
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())      # the state dict stays the reference's
    # unbound: the initial state, and forward is the plain expression
    nz = on.obs_normalizer
    assert nz.count == 0 and torch.equal(nz.mean, torch.zeros(37, dtype=torch.float64)) and torch.equal(nz.var, torch.ones(37, dtype=torch.float64))
    x = torch.randn(4, 37)
    assert torch.allclose(nz(x), x / (1.0 + 1e-2))
    sd = on.norm_state_dicts()
    assert set(sd) == {"obs_norm_state_dict", "critic_obs_norm_state_dict"}
    assert set(sd["obs_norm_state_dict"]) == {"mean", "var", "count", "eps", "until"}
    custom = ActorCritic(37, 19, 5, [24, 16], [24, 16], empirical_normalization=True, normalization_eps=0.0, normalization_until=1000)
    assert custom.obs_norm_spec == (0.0, 1000)
    for bad in (dict(normalization_eps=-1e-3), dict(normalization_eps=float("nan")), dict(normalization_until=-1), dict(normalization_until=2.5)):
        with pytest.raises(ValueError):
            ActorCritic(37, 19, 5, [24, 16], [24, 16], empirical_normalization=True, **bad)
    with pytest.raises(ValueError):          # checked whether the switch is on or not: a typo must not hide until it is
        ActorCritic(37, 19, 5, [24, 16], [24, 16], normalization_eps=-1.0)


def test_train_config_plumbing_both_places():
    from humanoid.algo.ppo.on_policy_runner import _split_policy_cfg, _check_norm_keys, NORM_KEYS
    pol = dict(actor_hidden_dims=[24, 16], critic_hidden_dims=[24, 16])
    assert _split_policy_cfg(pol, {}) == pol and _split_policy_cfg(pol, {}) is not pol
    assert _split_policy_cfg(pol, dict(empirical_normalization=True))["empirical_normalization"] is True       # rsl_rl's place
    assert _split_policy_cfg(dict(pol, empirical_normalization=True, normalization_eps=0.0), {}) == dict(pol, empirical_normalization=True, normalization_eps=0.0)
    assert _split_policy_cfg(dict(pol, empirical_normalization=True), dict(empirical_normalization=True))["empirical_normalization"] is True
    with pytest.raises(ValueError):
        _split_policy_cfg(dict(pol, empirical_normalization=False), dict(empirical_normalization=True))
    from humanoid.algo import ActorCritic
    ac = ActorCritic(37, 19, 5, **_split_policy_cfg(dict(pol, normalization_until=7), dict(empirical_normalization=True)))
    assert ac.obs_norm_spec == (1e-2, 7)
    # the reference's config classes gain no key (tests/test_api_surface.py compares them with the reference's dump)
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils import class_to_dict
    d = class_to_dict(XBotLCfgPPO())
    assert "empirical_normalization" not in d["policy"] and "empirical_normalization" not in d["runner"]
    # checkpoints: both mismatches are refused, naming the key
    both = {k: {} for k in NORM_KEYS}
    _check_norm_keys(both, True, "model_0.pt")
    _check_norm_keys({}, False, "model_0.pt")
    with pytest.raises(RuntimeError, match="obs_norm_state_dict"):
        _check_norm_keys(both, False, "model_0.pt")
    with pytest.raises(RuntimeError, match="obs_norm_state_dict"):
        _check_norm_keys({}, True, "model_0.pt")
    with pytest.raises(RuntimeError, match="critic_obs_norm_state_dict"):
        _check_norm_keys({NORM_KEYS[0]: {}}, True, "model_0.pt")
    # statistics saved under another eps or until: refused, naming the key and both values
    saved = {k: dict(eps=1e-2, until=None) for k in NORM_KEYS}
    _check_norm_keys(saved, True, "model_0.pt", (1e-2, None))
    with pytest.raises(RuntimeError, match="obs_norm_state_dict.*normalization_eps=0.01"):
        _check_norm_keys(saved, True, "model_0.pt", (1e-3, None))
    with pytest.raises(RuntimeError, match="normalization_until=None"):
        _check_norm_keys(saved, True, "model_0.pt", (1e-2, 1000))


def test_net_buffers_argument_is_validated_before_any_device_work():
    from hgym import check_obs_norm
    assert check_obs_norm(1e-2, None) == (1e-2, None) and check_obs_norm(0, 5) == (0.0, 5)
    for eps, until in ((-1.0, None), (float("inf"), None), (1e-2, -1), (1e-2, 0.5)):
        with pytest.raises(ValueError):
            check_obs_norm(eps, until)


def test_merge_restatement_on_a_hand_computed_example():
    """Two columns, two batches, by hand.  Batch 1 = rows (1, 10), (3, 10): mean (2, 10), population variance (1, 0); from mean 0 / var 1 /
    count 0 the rate is 1, so the state becomes exactly that.  Batch 2 = rows (5, 10), (5, 10), (5, 10), (9, 10): mean (6, 10), variance (3, 0);
    count 6, rate 2/3, d = (4, 0): mean = 2 + 8/3 = 14/3; var = 1 + 2/3 (3 - 1 + 4 (6 - 14/3)) = 1 + 2/3 (2 + 16/3) = 53/9 -- the
    population variance of the six values 1, 3, 5, 5, 5, 9 (mean 14/3, mean square 166/6 = 249/9, minus 196/9).  The constant column keeps 0."""
    s = ON.initial(2)
    assert s["count"] == 0 and list(s["mean"]) == [0, 0] and list(s["var"]) == [1, 1]
    s = ON.merge(s, [[1, 10], [3, 10]])
    assert s["count"] == 2 and list(s["mean"]) == [2, 10] and list(s["var"]) == [1, 0]
    s2 = ON.merge(s, [[5, 10], [5, 10], [5, 10], [9, 10]])
    assert s2["count"] == 6
    np.testing.assert_allclose(s2["mean"], [14 / 3, 10], rtol=1e-15)
    np.testing.assert_allclose(s2["var"], [53 / 9, 0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(s2["var"][0], np.var([1, 3, 5, 5, 5, 9]), rtol=1e-15)
    # until: a state that has seen enough rows skips the batch
    s3 = ON.merge(s, [[5, 10]], until=2)
    assert s3["count"] == 2 and list(s3["mean"]) == [2, 10]
    assert ON.merge(s, [[5, 10]], until=3)["count"] == 3
    # the kernels' floats: a constant column has the finite scale 1 / eps; eps = 0 and var = 4^k give exact powers of two
    m, sc = ON.derived(s2["mean"], s2["var"], 1e-2)
    assert m.dtype == np.float32 and sc[1] == np.float32(1.0 / float(np.float32(1e-2))) and np.isfinite(sc).all()
    _, p2 = ON.derived(np.zeros(5), 4.0 ** np.arange(-2, 3), 0.0)
    assert list(p2) == [4.0, 2.0, 1.0, 0.5, 0.25]


def test_fold_and_unfold_restatements_are_inverse_views_of_one_function():
    """W ((x - m) s) + b = (W s) x + (b - (W s) m) in float64 (fp32 operands: nothing is rounded to bf16 here), and the unfolded gradient
    of the folded layer is the chain rule's: dL/dW[r, c] = sum_rows g[r] (x[c] - m[c]) s[c]."""
    rng = np.random.default_rng(0)
    W, b = rng.standard_normal((6, 9)).astype(np.float32), rng.standard_normal(6).astype(np.float32)
    m, s = rng.standard_normal(9).astype(np.float32), (rng.random(9) + 0.5).astype(np.float32)
    x = rng.standard_normal((11, 9)).astype(np.float32)
    Wop, be, _ = ON.fold(W, b, m, s, "f32")
    y_fold = x.astype(np.float64) @ Wop.astype(np.float64).T + be
    y_norm = ON.normalise(x, m, s) @ W.astype(np.float64).T + b
    np.testing.assert_allclose(y_fold, y_norm, rtol=0, atol=1e-5)       # (Wop = fp32(W s): one fp32 rounding per weight)
    g = rng.standard_normal((11, 6))
    GW_folded, gb = g.T @ x.astype(np.float64), g.sum(axis=0)
    np.testing.assert_allclose(ON.unfold(GW_folded, gb, m, s), g.T @ ON.normalise(x, m, s), rtol=0, atol=1e-12)
    assert ON.bf16(np.float32([1.0, 1.00390625, 1.01171875, -3.0])).tolist() == [1.0, 1.0, 1.015625, -3.0]       # ties to even
