"""CPU: the host side of Random Network Distillation -- configuration parsing, the weight schedules at their edges,
the refusals that need no device, the checkpoint's keys, the float64 restatement of hgym_rnd_rewards (tests/rnd_common.py) against a
direct torch transcription, the size macro against its mirror, and hgym_rnd_rewards' argument checks (nothing is launched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnd_common as R
from hgym import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rnd():
    from humanoid.algo.ppo import rnd
    return rnd


# ------------------------------------------------------------------------------------------------ configuration
def test_defaults_and_the_default_state_columns():
    rnd = _rnd()
    c = rnd.parse_config({}, 705, 219, critic_frame=73)
    assert c["state"] == ("critic_obs", 146, 219)          # the newest of three 73-wide privileged frames, stacked oldest -> newest
    assert c["reward_normalization"] is True and c["state_normalization"] is False
    assert c["gamma"] == 0.99 and c["learning_rate"] == 1e-3 and c["weight"] == 0.0
    assert c["schedule"] == dict(mode="constant", weight=0.0, final_value=0.0, initial_step=0, final_step=0)
    assert set(c) == set(rnd.DEFAULTS) | {"schedule"}
    assert rnd.parse_config({}, 47, 19)["state"] == ("critic_obs", 0, 19)      # no frame width: the whole row
    assert rnd.parse_config(dict(state=("obs", 3, 50)), 705, 219)["state"] == ("obs", 3, 50)


@pytest.mark.parametrize("key", ["wieght", "symmetry", "num_output"])
def test_unknown_keys_are_refused_by_name(key):
    with pytest.raises(ValueError, match=key):
        _rnd().parse_config({key: 1}, 705, 219, 73)


@pytest.mark.parametrize("cfg, word", [
    (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"), (dict(weight="a"), "weight"),
    (dict(weight_schedule="linear"), "weight_schedule"), (dict(weight_schedule=dict(mode="cosine")), "mode"),
    (dict(weight_schedule=dict(final_step=3)), "weight_schedule"),
    (dict(weight_schedule=dict(mode="constant", final_step=3)), "final_step"),
    (dict(weight_schedule=dict(mode="step", final_step=3)), "final_value"),
    (dict(weight_schedule=dict(mode="step", final_step=3, final_value=0.1, initial_step=1)), "initial_step"),
    (dict(weight_schedule=dict(mode="step", final_step=-3, final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="step", final_step=3.5, final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="linear", initial_step=5, final_step=5, final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="linear", initial_step=6, final_step=5, final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="linear", initial_step=1, final_step=5, final_value=-0.1)), "final_value"),
    (dict(reward_normalization=1), "reward_normalization"), (dict(state_normalization="yes"), "state_normalization"),
    (dict(num_outputs=0), "num_outputs"), (dict(num_outputs=13), "num_outputs"), (dict(num_outputs=2.5), "num_outputs"),
    (dict(predictor_hidden_dims=[]), "predictor_hidden_dims"), (dict(target_hidden_dims=[64, 0]), "target_hidden_dims"),
    (dict(learning_rate=0.0), "learning_rate"), (dict(learning_rate=float("inf")), "learning_rate"),
    (dict(learning_rate="1e-3"), "learning_rate"), (dict(learning_rate=None), "learning_rate"), (dict(learning_rate=True), "learning_rate"),
    (dict(gamma=1.0), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma="0.9"), "gamma"), (dict(gamma=None), "gamma"), (dict(gamma=[0.9]), "gamma"),
    (dict(num_outputs="4"), "num_outputs"), (dict(num_outputs=None), "num_outputs"), (dict(weight=None), "weight"), (dict(weight=True), "weight"),
    (dict(weight_schedule=dict(mode="step", final_step="3", final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="step", final_step=None, final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="step", final_step=float("inf"), final_value=0.1)), "final_step"),
    (dict(weight_schedule=dict(mode="linear", initial_step="0", final_step=3, final_value=0.1)), "initial_step"),
    (dict(weight_schedule=dict(mode="step", final_step=3, final_value="0.1")), "final_value"),
    (dict(predictor_hidden_dims=["64"]), "predictor_hidden_dims"), (dict(state=("obs", "0", 5)), "state"), (dict(state=("obs", 0.0, 5)), "state"),
    (dict(state=("privileged", 0, 3)), "state"), (dict(state=("obs", 5, 5)), "state"), (dict(state=("obs", 0, 706)), "state"),
    (dict(state=("critic_obs", -1, 3)), "state"), (dict(state=[0, 5, 9]), "state"), (dict(state=("obs", 0)), "state"),
])
def test_refused_values(cfg, word):
    with pytest.raises(ValueError, match=word):
        _rnd().parse_config(cfg, 705, 219, 73)


def test_not_a_dict_is_refused():
    with pytest.raises(ValueError, match="rnd_cfg"):
        _rnd().parse_config([("weight", 1.0)], 705, 219, 73)


# ------------------------------------------------------------------------------------------------ schedules
def test_schedules_at_their_edges():
    rnd = _rnd()
    const = rnd.parse_schedule(0.5, None)
    assert [rnd.schedule_weight(const, c) for c in (0, 1, 10 ** 9)] == [0.5] * 3
    step = rnd.parse_schedule(0.5, dict(mode="step", final_step=10, final_value=0.125))
    assert [rnd.schedule_weight(step, c) for c in (9, 10, 11)] == [0.5, 0.125, 0.125]
    lin = rnd.parse_schedule(1.0, dict(mode="linear", initial_step=10, final_step=20, final_value=0.25))
    got = [rnd.schedule_weight(lin, c) for c in (9, 10, 11, 19, 20, 21)]
    assert got == [1.0, 1.0, 1.0 + (0.25 - 1.0) * 1.0 / 10.0, 1.0 + (0.25 - 1.0) * 9.0 / 10.0, 0.25, 0.25]
    assert got[2] == 0.925 and got[3] == pytest.approx(0.325, abs=1e-15)
    up = rnd.parse_schedule(0.0, dict(mode="linear", initial_step=0, final_step=3, final_value=3.0))      # a rising line is allowed
    assert [rnd.schedule_weight(up, c) for c in range(5)] == [0.0, 1.0, 2.0, 3.0, 3.0]
    # the test-side schedule (written from the header) and the product's agree everywhere around the edges
    for s in (const, step, lin, up):
        kw = dict(schedule=rnd.SCHEDULES.index(s["mode"]), w0=s["weight"], final_value=s["final_value"], initial_step=s["initial_step"],
                  final_step=s["final_step"])
        for c in range(0, 25):
            assert R.weight(c, **kw) == rnd.schedule_weight(s, c)
    assert (R.CONSTANT, R.STEP, R.LINEAR) == (L.RND_CONSTANT, L.RND_STEP, L.RND_LINEAR) == tuple(range(3))


# ------------------------------------------------------------------------------------------------ PPO and the refusals
def test_rnd_is_off_by_default():
    from humanoid.algo import PPO, Distillation
    assert PPO.rnd is None and Distillation.rnd is None and "rnd" in vars(PPO)
    import inspect
    assert "rnd" not in inspect.signature(PPO.__init__).parameters      # a class attribute, like symmetry


def test_check_setup_refusals():
    rnd = _rnd()
    rnd.check_setup()                                                       # the defaults pass
    rnd.check_setup(1, object(), False)                                     # the mirror loss without augmentation is fine
    with pytest.raises(ValueError, match="one rank"):
        rnd.check_setup(world=2)
    with pytest.raises(ValueError, match="symmetry_augmentation"):
        rnd.check_setup(1, object(), True)
    with pytest.raises(ValueError, match="Distillation"):
        rnd.check_setup(distillation=True)


def test_the_runner_takes_rnd_cfg_out_of_the_algorithm_block():
    from humanoid.algo.ppo import on_policy_runner as O
    kwargs, sym = O._split_algorithm_cfg(dict(gamma=0.9, rnd_cfg=dict(weight=1.0)))
    assert kwargs == dict(gamma=0.9) and sym is False and O.RND_KEY == "rnd_cfg" and O.RND_STATE_KEY == "rnd_state_dict"


def test_default_train_config_gains_no_key():
    from humanoid.envs import task_registry
    _, train_cfg = task_registry.get_cfgs("humanoid_ppo")
    assert not hasattr(train_cfg.algorithm, "rnd_cfg")


# ------------------------------------------------------------------------------------------------ the module and its checkpoint
def _module(seed=7, **cfg):
    from humanoid.algo import RandomNetworkDistillation
    return RandomNetworkDistillation(47, 19, dict(dict(predictor_hidden_dims=[24, 16], target_hidden_dims=[32], num_outputs=5), **cfg), seed=seed)


def test_module_is_seeded_and_the_target_is_frozen():
    a, b, c = _module(7), _module(7), _module(8)
    torch.manual_seed(123)      # (the global generator plays no part)
    d = _module(7)
    for x, y, z, w in zip(a.state_dict().values(), b.state_dict().values(), c.state_dict().values(), d.state_dict().values()):
        assert torch.equal(x, y) and torch.equal(x, w) and not torch.equal(x, z)
    assert all(not p.requires_grad for p in a.target.parameters()) and all(p.requires_grad for p in a.predictor.parameters())
    assert a.num_states == 19 and a.num_outputs == 5 and (a.source, a.start, a.stop) == ("critic_obs", 0, 19)
    assert a.predictor[0].in_features == 19 and a.predictor[-1].out_features == 5 and a.target[-1].out_features == 5
    assert not torch.equal(a.predictor[0].weight, a.target[0].weight[:24]) and not a.bound


def test_rnd_state_dict_keys_and_load_refusals_by_name():
    rnd = _rnd()
    m = _module()
    sd = m.rnd_state_dict()
    assert tuple(sd) != () and set(sd) == set(rnd.STATE_DICT_KEYS)
    assert set(rnd.STATE_DICT_KEYS) == {"predictor", "target", "predictor_adam_m", "predictor_adam_v", "predictor_opt_state", "block", "num_envs",
                                        "state_norm"}
    assert set(sd["predictor"]) == {"0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"} and set(sd["target"]) == {"0.weight", "0.bias", "2.weight", "2.bias"}
    other = _module(seed=9)
    other.load_rnd_state_dict(sd)
    for x, y in zip(m.state_dict().values(), other.state_dict().values()):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError, match="model_5.pt carries rnd_state_dict"):
        rnd.check_state_dict(sd, "model_5.pt", False)
    with pytest.raises(RuntimeError, match="model_5.pt has no rnd_state_dict"):
        rnd.check_state_dict(None, "model_5.pt", True)
    with pytest.raises(RuntimeError, match="64 envs, this run has 128"):
        rnd.check_state_dict(dict(sd, num_envs=64), "model_5.pt", True, 128)
    with pytest.raises(RuntimeError, match="lacks block"):
        rnd.check_state_dict({k: v for k, v in sd.items() if k != "block"}, "model_5.pt", True)
    rnd.check_state_dict(None, "model_5.pt", False)
    rnd.check_state_dict(dict(sd, num_envs=128), "model_5.pt", True, 128)


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_transcription(pred, target, rewards, G, stats, counter, gamma, sched, normalize):
    """rsl_rl's forms, with this repository's one merge per rollout: torch.linalg.norm, a Python loop for the discounted average."""
    pred, target = torch.as_tensor(pred, dtype=torch.float64), torch.as_tensor(target, dtype=torch.float64)
    T, n, _ = pred.shape
    err = torch.linalg.norm(target - pred, dim=2)
    G = torch.as_tensor(G, dtype=torch.float64).clone()
    rows = []
    for t in range(T):
        G = G * gamma + err[t]
        rows.append(G.clone())
    allG = torch.stack(rows)
    mean, var, count = stats
    nb = float(allG.numel())
    mu_b, var_b = float(allG.mean()), float(allG.var(unbiased=False))
    tot = count + nb
    delta = mu_b - mean
    new_mean = mean + delta * nb / tot
    # Chan's parallel form, as rsl_rl's normaliser merges: M2 = var * count + var_b * nb + delta^2 * count * nb / tot
    new_var = (var * count + var_b * nb + delta * delta * count * nb / tot) / tot
    std = new_var ** 0.5
    out = torch.as_tensor(rewards, dtype=torch.float64).clone()
    intr = torch.empty(T, n, dtype=torch.float64)
    for t in range(T):
        w = R.weight(counter + t + 1, **sched)
        scale = float(np.float32(w / std if (normalize and std > 0) else w))
        intr[t] = err[t] * scale
        out[t] += intr[t]
    return err, G, (new_mean, new_var, tot), intr, out


@pytest.mark.parametrize("T, n, K, normalize", [(1, 1, 1, True), (5, 17, 3, True), (4, 65, 12, False), (3, 257, 33, True)])
def test_restatement_equals_a_direct_torch_transcription(T, n, K, normalize):
    rng = np.random.default_rng(T * 1000 + n)
    sched = dict(schedule=R.LINEAR, w0=1.5, final_value=0.25, initial_step=2, final_step=9)
    state = R.fresh_state(n)
    G0, stats0, counter0 = state["G"].copy(), (0.0, 1.0, 0.0), 0
    for call in range(3):      # the carry across rollouts as well
        pred, target = rng.standard_normal((T, n, K)).astype(np.float32), rng.standard_normal((T, n, K)).astype(np.float32)
        rewards = rng.standard_normal((T, n)).astype(np.float32)
        ref = R.reference(pred, target, rewards, state, gamma=0.9, normalize=normalize, **sched)
        err, G, stats, intr, out = _torch_transcription(pred, target, rewards, G0, stats0, counter0, 0.9, sched, normalize)
        np.testing.assert_allclose(ref["err"], err.numpy(), rtol=1e-14)
        np.testing.assert_allclose(ref["state"]["G"], G.numpy(), rtol=1e-13)
        assert ref["state"]["mean"] == pytest.approx(stats[0], rel=1e-12) and ref["state"]["var"] == pytest.approx(stats[1], rel=1e-10)
        assert ref["state"]["count"] == stats[2] == (call + 1) * T * n and ref["state"]["counter"] == (call + 1) * T
        np.testing.assert_allclose(ref["intrinsic"], intr.numpy(), rtol=1e-6)      # scale is an fp32 number of a std that agrees to 1e-10
        np.testing.assert_allclose(rewards.astype(np.float64) + ref["intrinsic"], out.numpy(), rtol=1e-6, atol=1e-6)
        state, G0, stats0, counter0 = ref["state"], G.numpy(), stats, counter0 + T
    if not normalize:
        assert np.all(ref["scale"] == np.float32(0.25))      # past final_step: the weight alone


def test_restatement_by_hand():
    """Two envs, two steps, numbers small enough to follow: errors 3, 4 / 0, 5; gamma = 0.5."""
    pred = np.zeros((2, 2, 2), dtype=np.float32)
    target = np.array([[[3, 0], [0, 4]], [[0, 0], [3, 4]]], dtype=np.float32)
    ref = R.reference(pred, target, np.ones((2, 2), dtype=np.float32), R.fresh_state(2), gamma=0.5, schedule=R.STEP, w0=2.0, final_value=1.0,
                      final_step=2)
    assert ref["err"].tolist() == [[3.0, 4.0], [0.0, 5.0]]
    assert ref["G_all"].tolist() == [[3.0, 4.0], [1.5, 7.0]] and ref["state"]["G"].tolist() == [1.5, 7.0]
    mu = 15.5 / 4
    var_b = (9 + 16 + 2.25 + 49) / 4 - mu * mu
    # merged into (0, 1, 0): rate = 1, mean = mu, var = 1 + (var_b - 1 + mu * (mu - mu)) = var_b
    assert ref["state"]["mean"] == mu and ref["state"]["var"] == pytest.approx(var_b, rel=1e-15) and ref["state"]["count"] == 4.0
    assert ref["scale"].tolist() == [float(np.float32(2.0 / var_b ** 0.5)), float(np.float32(1.0 / var_b ** 0.5))] and ref["w_last"] == 1.0
    assert ref["state"]["counter"] == 2


# ------------------------------------------------------------------------------------------------ the C side that needs no device
def test_size_macro_and_its_mirrors():
    header = open(os.path.join(ROOT, "include", "hgym.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"\\\n", " ", header))
    for macro in ("#define HGYM_RND_HEADER 16", "#define HGYM_RND_ENVS_PER_PARTIAL 64", "#define HGYM_RND_APPLY_WGS 1024", "#define HGYM_RND_MAX_OUTPUTS 64",
                  "#define HGYM_RND_ROWS_PER_WG 64",
                  "#define HGYM_RND_BLOCK_DOUBLES(n) ((size_t)HGYM_RND_HEADER + (size_t)(n) + 2 * (((size_t)(n) + HGYM_RND_ENVS_PER_PARTIAL - 1) / "
                  "HGYM_RND_ENVS_PER_PARTIAL) + 2 * (size_t)HGYM_RND_APPLY_WGS)"):
        assert macro in text, macro
    for n in (1, 2, 255, 256, 257, 4097):
        assert R.block_doubles(n) == L.rnd_block_doubles(n) == R.host_block(n).size
    assert R.block_doubles(1) == 16 + 1 + 2 + 2048 and R.block_doubles(257) == 16 + 257 + 10 + 2048
    with pytest.raises(AssertionError):
        L.rnd_block(3, "cpu")      # the block is written by hgym_rnd_block_init: a device call
    hdr = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("MEAN", "VAR", "COUNT", "COUNTER", "SUM_INTRINSIC", "SUM_REWARDS", "WEIGHT_LAST", "STD", "ROWS", "TICKET_SCAN", "TICKET_APPLY",
                 "HEADER", "MAX_OUTPUTS", "CONSTANT", "STEP", "LINEAR", "ROWS_PER_WG", "ENVS_PER_PARTIAL", "APPLY_WGS"):
        assert int(re.search(r"#define\s+HGYM_RND_%s\s+(\d+)" % name, hdr).group(1)) == getattr(L, "RND_" + name), name
    assert (R.HEADER, R.ENVS_PER_PARTIAL, R.ROWS_PER_WG, R.APPLY_WGS, R.MAX_OUTPUTS) == (L.RND_HEADER, L.RND_ENVS_PER_PARTIAL, L.RND_ROWS_PER_WG,
                                                                                        L.RND_APPLY_WGS, L.RND_MAX_OUTPUTS)


def test_struct_and_symbols():
    assert L.STRUCTS["HgymRndConfig"] is L.RndConfig and C.sizeof(L.RndConfig) == L.lib.hgym_sizeof(b"HgymRndConfig") == 48
    for sym in ("hgym_rnd_block_init", "hgym_rnd_rewards"):
        assert sym in L.SYMBOLS and hasattr(L.lib, sym)
    assert L.lib.hgym_version() == 9


def _call(T=2, n=3, K=4, cfg=None, null=None):
    bufs = {k: torch.zeros(64) for k in ("pred", "target", "rewards", "err", "intrinsic")}
    block = torch.from_numpy(R.host_block(max(n, 1)))
    cfg = cfg if cfg is not None else L.RndConfig(0.99, 1.0, 0.0, 0, 0, L.RND_CONSTANT, 1)
    p = {k: (None if k == null else L.fptr(v)) for k, v in bufs.items()}
    return L.lib.hgym_rnd_rewards(T, n, K, p["pred"], p["target"], p["rewards"], p["err"], p["intrinsic"], None if null == "cfg" else C.byref(cfg),
                                  None if null == "block" else L.f64ptr(block), None)


@pytest.mark.parametrize("kw", [dict(T=0), dict(n=0), dict(K=0), dict(K=65), dict(T=-1)] +
                         [dict(null=k) for k in ("pred", "target", "rewards", "err", "intrinsic", "cfg", "block")] +
                         [dict(cfg=c) for c in ((1.0, 1.0, 0.0, 0, 0, 0, 1), (-0.1, 1.0, 0.0, 0, 0, 0, 1), (float("nan"), 1.0, 0.0, 0, 0, 0, 1),
                                                (0.9, -1.0, 0.0, 0, 0, 0, 1), (0.9, float("inf"), 0.0, 0, 0, 0, 1), (0.9, float("nan"), 0.0, 0, 0, 0, 1),
                                                (0.9, 1.0, -1.0, 0, 5, 1, 1), (0.9, 1.0, float("nan"), 0, 5, 2, 1), (0.9, 1.0, 0.5, 5, 5, 2, 1),
                                                (0.9, 1.0, 0.5, 6, 5, 2, 1), (0.9, 1.0, 0.0, 0, 0, 3, 1), (0.9, 1.0, 0.0, 0, 0, -1, 1),
                                                (0.9, 1.0, 0.0, 0, 0, 0, 2))])
def test_bad_arguments_are_refused_before_anything_is_launched(kw):
    """Host pointers here: a call that got as far as a launch would not return HGYM_E_BADARG."""
    if "cfg" in kw:
        kw = dict(cfg=L.RndConfig(*kw["cfg"]))
    assert _call(**kw) == -1 and L.lib.hgym_last_error()
    assert L.lib.hgym_rnd_block_init(0, L.f64ptr(torch.zeros(4, dtype=torch.float64)), None) == -1
    assert L.lib.hgym_rnd_block_init(4, None, None) == -1
