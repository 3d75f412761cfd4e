"""-m gpu: value-target normalisation through the drop-in stack (PPO.value_normalization, the train config's algorithm.value_normalization;
DESIGN.md section 31), at 64 envs, rollouts of 8 steps, 2 minibatches x 2 epochs.

  * off means absent: no checkpoint key, a `value_norm` graph-key entry of None, the log block at its old size;
  * one iteration issued step by step against the restatement (tests/value_norm_common.py): the stored values are denormalise(v) bitwise,
    the block after compute_returns is the merge of the raw returns' statistics to 1e-10, `returns` and `values` are the fp32 map of the
    raw columns bitwise;
  * the captured update replays what the eager one does and the captured stepwise rollout what the eager one does, bit for bit over 3
    iterations, on every loop plan; the one-launch rollout takes the deferred critic;
  * checkpoints: both save paths carry the same entry, a round trip, 2 + 2 iterations with exact resume equal 4, load()'s three refusals;
  * the options combined; init_storage's refusals."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import value_norm_common as V
from hgym import _lib as L

pytestmark = pytest.mark.gpu
TASK, N, T = "humanoid_ppo", 64, 8
KEY = "value_norm_state_dict"
KNOBS = ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK", "HGYM_ASYNC_SAVE")
# loop plans of the runner: the knobs OnPolicyRunner reads once per learn()
PLANS = {"default": {}, "unfused": {"HGYM_FUSE_ROLLOUT": "0"}, "no-rollout-graph": {"HGYM_GRAPH": "0"}, "sync": {"HGYM_ASYNC": "0"},
         "deferred-critic": {"HGYM_ROLLOUT_CRITIC": "deferred"}, "host-log": {"HGYM_LOG_SINK": "0"}}
# the options that combine, in sets init_storage accepts (PPO.smoothness refuses PPO.symmetry, PPO.rnd the augmentation: as before)
COMBINED = {
    "mirror-loss+rnd": dict(alg=dict(symmetry=True, symmetry_augmentation=False, mirror_loss_coef=0.5, advantage_normalization="minibatch",
                                     rnd_cfg=dict(weight=0.5, predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128])),
                            policy=dict(empirical_normalization=True)),
    "augmentation+mirror-loss": dict(alg=dict(symmetry=True, mirror_loss_coef=0.5, advantage_normalization="minibatch", use_clipped_value_loss=False),
                                     policy=dict(empirical_normalization=True, noise_std_type="log")),
    "smoothness+rnd+aux": dict(task="humanoid_dwl_ppo",
                               alg=dict(smoothness_cfg=dict(temporal_coef=2.0, spatial_coef=4.0), advantage_normalization="none",
                                        rnd_cfg=dict(weight=0.5, predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128])),
                               policy=dict(empirical_normalization=True, noise_std_type="log")),
}


def _runner(tmp=None, on=True, eps=None, seed=31, exact=False, save_interval=50, combined=None):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    extra = COMBINED.get(combined, {})
    task = extra.get("task", TASK)
    args = get_args(["--task=" + task, "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=task))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if on:
        train_cfg.algorithm.value_normalization = True
    if eps is not None:
        train_cfg.algorithm.value_normalization_eps = eps
    for k, v in extra.get("alg", {}).items():
        setattr(train_cfg.algorithm, k, v)
    for k, v in extra.get("policy", {}).items():
        setattr(train_cfg.policy, k, v)
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name=task, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert (runner.alg.value_normalizer is not None) == on and getattr(PPO, "value_normalization", False) is False
    return runner


def _state(runner):
    torch.cuda.synchronize()
    net, st, vn = runner.alg.net, runner.alg.storage, runner.alg.value_normalizer
    out = [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all[0].clone()]
    if vn is not None:
        out.append(vn.block.clone())
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _clean(monkeypatch, **knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------- the default
def test_off_means_absent(monkeypatch, tmp_path):
    from humanoid.algo.ppo import checkpoint as ckpt
    _clean(monkeypatch)
    r = _runner(tmp_path / "off", on=False)
    alg, st = r.alg, r.alg.storage
    assert alg.value_normalizer is None and alg._options == () and alg.last_value_norm is None
    assert dict(alg.update_graph_key()).get("value_norm") is None
    assert alg.rollout_graph_key() == (id(st), alg.gamma, st._obs_bf16 is not None)
    assert alg.log_block().numel() == alg.net.opt_state.numel() == L.OPT_STATE
    assert KEY not in ckpt.extra_entries(alg)
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    r.wait_for_saves()
    saved = torch.load(os.path.join(r.log_dir, "model_1.pt"), map_location="cpu")
    assert list(saved) == ["model_state_dict", "optimizer_state_dict", "iter", "infos"]
    assert not any(k[0].startswith("Policy/value_norm") for k in alg.log_scalars())


# ---------------------------------------------------------------------------------------------- one iteration, step by step
def _host_floats(block, eps):
    b = block.cpu()
    return b[1].float(), torch.sqrt(b[2]).float() + torch.tensor(eps, dtype=torch.float32)


def test_one_iteration_against_the_restatement(monkeypatch):
    _clean(monkeypatch)
    r = _runner(eps=0.05)
    env, alg, st = r.env, r.alg, r.alg.storage
    vn = alg.value_normalizer
    assert vn.eps == 0.05 and [float(x) for x in vn.block.cpu()] == list(V.INITIAL) and vn.last_values.shape == (N, 1)
    assert alg.value_normalizer.count == 0 and vn.scratch.numel() == V.scratch_doubles(T * N)
    before = (300.0, 0.7, 2.3)      # a state that already holds data: the maps are not the identity
    vn.block.copy_(torch.tensor(before, dtype=torch.float64))
    mean_f, scale_f = _host_floats(vn.block, 0.05)
    seen = []
    real = vn.denormalize

    def recorded(v, out=None):
        v_in = v.clone()
        res = real(v, out)
        seen.append((v_in.cpu().view(-1), res.clone().cpu().view(-1)))
        return res
    monkeypatch.setattr(vn, "denormalize", recorded)
    with torch.inference_mode():
        obs, priv = env.get_observations(), env.get_privileged_observations()
        for s in range(T):
            obs, priv, rew, dones, infos = env.step(alg.act(obs.clone(), priv.clone()))
            assert torch.equal(alg.transition.values, st.values[s])      # transition.values is the slot, already raw
            alg.process_env_step(rew, dones, infos)
        torch.cuda.synchronize()
        assert len(seen) == T
        for s, (v, V_raw) in enumerate(seen):      # values before GAE: denormalise(v), bitwise
            want = v * scale_f
            want = want + mean_f
            assert torch.equal(V_raw.view(torch.int32), want.view(torch.int32)) and torch.equal(st.values[s].cpu().view(-1), V_raw), s
        assert float(torch.stack([v for v, _ in seen]).abs().max()) > 0.0
        # the raw returns: the storage's own GAE with the option's passes skipped (RolloutStorage.compute_returns runs none of them)
        v_last = alg.actor_critic.evaluate(priv).clone().cpu().view(-1)      # what the critic outputs: normalised
        V_last = v_last * scale_f
        V_last = (V_last + mean_f).to("cuda")
        st.compute_returns(V_last.view(N, 1), alg.gamma, alg.lam, normalize=False)
        torch.cuda.synchronize()
        raw_returns, raw_values, raw_adv = st.returns.clone().cpu(), st.values.clone().cpu(), st.advantages.clone()
        alg.compute_returns(priv)
        torch.cuda.synchronize()
    assert len(seen) == T + 1 and torch.equal(seen[-1][0], v_last) and torch.equal(seen[-1][1].view(torch.int32), V_last.cpu().view(torch.int32))
    assert torch.equal(vn.last_values.cpu().view(-1), V_last.cpu())
    # the block: the restatement's merge of the raw returns' statistics
    batch = V.batch_stats(raw_returns.numpy())
    want = V.merge(before, batch)
    got = [float(x) for x in vn.block.cpu()]
    errs = [V.rel(g, w) for g, w in zip(got, want)]
    print("block after compute_returns %r, restatement %r, relative errors %r" % (got, want, errs))
    assert got[0] == want[0] == 300.0 + T * N and max(errs) <= 1e-10
    assert max(V.rel(float(g), w) for g, w in zip(vn.scratch[:3].cpu(), batch)) <= 1e-10
    # returns and values: the fp32 map of the raw columns under the NEW statistics, bitwise; the advantages are untouched by the option
    m2, s2 = _host_floats(vn.block, 0.05)
    assert float(m2) != float(mean_f)
    for name, raw in (("returns", raw_returns), ("values", raw_values)):
        assert torch.equal(getattr(st, name).cpu().view(torch.int32), ((raw - m2) / s2).view(torch.int32)), name
    adv = raw_adv.double()
    assert torch.allclose(st.advantages.double(), (adv - adv.mean()) / (adv.std() + 1e-8), rtol=1e-4, atol=2e-5)
    assert alg.value_normalizer.count == 300 + T * N and float(alg.value_normalizer.mean) == got[1] and float(alg.value_normalizer.std) == math.sqrt(got[2])
    value_loss, surrogate = alg.update(sync=True)
    assert np.isfinite(value_loss) and np.isfinite(surrogate) and bool(torch.isfinite(alg.net.params).all())
    assert alg.last_value_norm == dict(count=got[0], mean=got[1], var=got[2], std=math.sqrt(got[2]))
    assert alg.log_scalars()[-2:] == [("Policy/value_norm_mean", got[1]), ("Policy/value_norm_std", math.sqrt(got[2]))]
    assert alg.log_block().numel() == L.OPT_STATE + 3


# ---------------------------------------------------------------------------------------------- the loop plans
@pytest.mark.parametrize("plan", list(PLANS))
def test_captured_equals_eager_on_every_plan(monkeypatch, tmp_path, plan):
    from humanoid.algo.ppo.on_policy_runner import _plan_loop
    _clean(monkeypatch, **PLANS[plan])
    a = _runner(tmp_path / "a")
    fused = _plan_loop(a.env, a.alg, a.device, True).fuse
    a.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    a.wait_for_saves()
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(tmp_path / "b")
    b.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    b.wait_for_saves()
    assert b._update_graph is None
    assert _same(sa, _state(b)), "plan %s: the captured update and the eager one differ" % plan
    print("plan %s: update graph %s, rollout graph %s, fuse %s" % (plan, a._update_graph is not None, a._graph is not None, fused))
    if plan == "default":
        assert a._update_graph is not None and a._graph is not None and a.alg.update_capturable()
    if plan == "unfused":      # the captured stepwise rollout (with its denormalise launches) against the eager one
        assert fused is None and a._graph is not None
        monkeypatch.setenv("HGYM_GRAPH", "0")
        c = _runner(tmp_path / "c")
        c.learn(num_learning_iterations=3, init_at_random_ep_len=True)
        c.wait_for_saves()
        assert c._graph is None and _same(sa, _state(c)), "the captured stepwise rollout and the eager one differ"
    block = [float(x) for x in a.alg.value_normalizer.block.cpu()]
    assert block[0] == 3.0 * T * N and np.isfinite(block[1]) and block[2] > 0.0
    assert all(bool(torch.isfinite(t.double()).all()) for t in sa)
    # the host state a replay must leave, as tests/test_runner_graph_gpu.py compares it
    for r in (a, b):
        assert r.alg.storage.step == 0 and r.alg._deferred_ready is False and r.alg._perm_draws == 3


def test_keys_change_with_the_option(monkeypatch):
    _clean(monkeypatch)
    on, off = _runner().alg, _runner(on=False).alg
    key, key_off = on.update_graph_key(), off.update_graph_key()
    vn = on.value_normalizer
    assert dict(key)["value_norm"] == (1e-2, vn.block.data_ptr(), vn.scratch.data_ptr()) and dict(key_off)["value_norm"] is None
    assert [n for n, _ in key] == [n for n, _ in key_off]
    assert on.rollout_graph_key()[:3] == (id(on.storage), on.gamma, True) and len(on.rollout_graph_key()) == 4 and len(off.rollout_graph_key()) == 3
    vn.eps = 0.5
    assert on.update_graph_key() != key and on.rollout_graph_key()[3][0] == 0.5      # another eps re-captures both graphs


def test_the_one_launch_rollout_takes_the_deferred_critic(monkeypatch):
    from humanoid.algo.ppo.on_policy_runner import _plan_loop
    _clean(monkeypatch)
    on, off = _runner(), _runner(on=False)
    reported = off.env.rollout_fused_mode(off.alg.net)
    assert reported == "inline"      # 64 envs: two tiles of each kind fit the chip
    assert _plan_loop(off.env, off.alg, off.device, False).fuse == reported
    assert _plan_loop(on.env, on.alg, on.device, False).fuse == "deferred" and _plan_loop(on.env, on.alg, on.device, True).fuse == "deferred"
    monkeypatch.setenv("HGYM_ROLLOUT_CRITIC", "deferred")
    assert _plan_loop(off.env, off.alg, off.device, False).fuse == "deferred" == _plan_loop(on.env, on.alg, on.device, False).fuse
    monkeypatch.setenv("HGYM_FUSE_ROLLOUT", "0")
    assert _plan_loop(off.env, off.alg, off.device, False).fuse is None and _plan_loop(on.env, on.alg, on.device, False).fuse is None


# ---------------------------------------------------------------------------------------------- checkpoints
def test_both_save_paths_carry_the_entry_and_a_round_trip(monkeypatch, tmp_path):
    _clean(monkeypatch)
    a = _runner(tmp_path / "a")
    a.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    a.wait_for_saves()
    block = a.alg.value_normalizer.block.cpu()
    entry = dict(count=float(block[0]), mean=float(block[1]), var=float(block[2]), eps=1e-2)
    background = torch.load(os.path.join(a.log_dir, "model_2.pt"), map_location="cpu")
    assert list(background)[-1] == KEY and background[KEY] == entry and entry["count"] == 2.0 * T * N
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")
    a.save(str(tmp_path / "blocking.pt"))
    blocking = torch.load(str(tmp_path / "blocking.pt"), map_location="cpu")
    assert list(blocking) == list(background) and blocking[KEY] == entry
    monkeypatch.delenv("HGYM_ASYNC_SAVE")
    b = _runner(tmp_path / "b", seed=32)
    assert b.alg.value_normalizer.count == 0
    b.load(os.path.join(a.log_dir, "model_2.pt"))
    assert torch.equal(b.alg.value_normalizer.block.cpu().view(torch.int64), block.view(torch.int64))
    assert b.alg.value_normalizer.state_dict() == entry and torch.equal(b.alg.net.params, a.alg.net.params)


def test_exact_resume_from_the_middle(tmp_path, monkeypatch):
    _clean(monkeypatch)
    u = _runner(tmp_path / "u", exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    r = _runner(tmp_path / "r", exact=True, save_interval=50)
    r.load(os.path.join(u.log_dir, "model_1.pt"))
    assert r.current_learning_iteration == 2 and r.alg.value_normalizer.count == 2 * T * N
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(_state(u), _state(r))


def test_load_refuses_the_other_kind_of_checkpoint(monkeypatch, tmp_path):
    _clean(monkeypatch)
    on, off = _runner(tmp_path / "on"), _runner(tmp_path / "off", on=False)
    on.save(str(tmp_path / "on.pt"))
    off.save(str(tmp_path / "off.pt"))
    params = on.alg.net.params.clone()
    with pytest.raises(RuntimeError, match="off.pt has no `value_norm_state_dict`"):
        on.load(str(tmp_path / "off.pt"))
    with pytest.raises(RuntimeError, match="on.pt carries `value_norm_state_dict`"):
        off.load(str(tmp_path / "on.pt"))
    other = _runner(tmp_path / "eps", eps=0.05)
    with pytest.raises(RuntimeError, match=r"`value_norm_state_dict` was saved with value_normalization_eps=0.01; this run was built with 0.05"):
        other.load(str(tmp_path / "on.pt"))
    assert torch.equal(on.alg.net.params, params)      # refused before anything is changed
    on.load(str(tmp_path / "on.pt"))


# ---------------------------------------------------------------------------------------------- the options combined
@pytest.mark.parametrize("combined", list(COMBINED))
def test_everything_else_on(monkeypatch, combined):
    _clean(monkeypatch)
    a = _runner(combined=combined)
    alg = a.alg
    assert alg._obs_norm is not None and alg._adv_mode == COMBINED[combined]["alg"]["advantage_normalization"]
    if combined == "mirror-loss+rnd":
        assert alg._rnd is not None and alg._mirror_loss.coef == 0.5 and not alg._augment and alg._symmetry is not None
    elif combined == "augmentation+mirror-loss":
        assert alg._augment and alg._mirror_loss.coef == 0.5 and not alg.use_clipped_value_loss and alg.storage.mirrored
    else:
        assert alg._rnd is not None and alg._smooth is not None and alg._ppo_cfg.aux_coef > 0.0
    a.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    sa = _state(a)
    print("%s: update graph %s" % (combined, a._update_graph is not None))
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(combined=combined)
    b.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    assert b._update_graph is None and _same(sa, _state(b))
    assert all(bool(torch.isfinite(t.double()).all()) for t in sa)
    st = b.alg.storage
    if st.mirrored:      # the mirrored half holds the normalised columns too (storage.mirror() runs behind compute_returns)
        for name in ("values", "returns"):
            c = st._col_store[name]
            assert torch.equal(c[T + 1:], c[:T]) or not b.alg._augment
    parts = b.alg._log.split(b.alg.log_block().cpu())
    assert list(parts)[-1] == "value_norm" and float(parts["value_norm"][0]) == 2.0 * T * N


# ---------------------------------------------------------------------------------------------- refusals
def test_init_storage_refusals(monkeypatch):
    from humanoid.algo import PPO, Distillation
    _clean(monkeypatch)
    r = _runner(on=False)
    ac = r.alg.actor_critic
    alg = PPO(ac, num_mini_batches=2, device=r.device)
    alg.value_normalization = True
    alg._world = 2
    with pytest.raises(ValueError, match=r"PPO.value_normalization runs on one rank \(world size 2\)"):
        alg.init_storage(N, T, [705], [219], [12])
    alg._world, alg.value_normalization_eps = 1, -1.0
    with pytest.raises(ValueError, match="value_normalization_eps=-1.0: must be finite and >= 0"):
        alg.init_storage(N, T, [705], [219], [12])
    d = Distillation(ac, gradient_length=4, device=r.device)
    d.value_normalization = True
    with pytest.raises(ValueError, match="PPO.value_normalization does not support Distillation"):
        d.init_storage(N, T, [705], [219], [12])
