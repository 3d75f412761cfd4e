"""-m gpu: guidance by a frozen teacher through the drop-in stack (PPO.guidance, OnPolicyRunner's guidance_cfg), at 64
envs, rollouts of 8 steps, XBot-L's widths, 2 minibatches x 2 epochs.

  * the captured update replays what the eager update does, bit for bit, across a linear schedule that runs out mid-run -- the switch to
    the plain update (one re-capture through the changed graph key) included; the coefficient logged at every iteration is the twin's;
  * after the run-out the parameters follow an unguided continuation bit for bit;
  * an exact resume mid-schedule equals the uninterrupted run, and needs no teacher file;
  * the option off has nothing of the feature: the parent's launches, graph-key values and log-block size;
  * combined once with RND + value normalisation + empirical_normalization;
  * the teacher's pass in ragged pieces equals hgym_mlp_forward, bit for bit;
  * with a large constant coefficient and a fixed learning rate the MSE between student and teacher means on fixed rows falls over ten
    updates and ends lower than in the same run unguided;
  * init_storage's refusals and load()'s."""
import copy
import os

import numpy as np
import pytest
import torch

from hgym import _lib as L

pytestmark = pytest.mark.gpu
TASK, N, T = "humanoid_ppo", 64, 8
FINAL = 3      # the linear schedule of most cases: 2.0 at update 0, 0 from update 3 on
LINEAR = dict(coef=2.0, coef_schedule=dict(mode="linear", initial_step=0, final_step=FINAL, final_value=0.0))
PLANS = {"default": {}, "unfused": {"HGYM_FUSE_ROLLOUT": "0"}, "sync": {"HGYM_ASYNC": "0"}}
KNOBS = ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK")


def _teacher(seed=77, hidden=(512, 256, 128), no=705, A=12):
    """A PPO checkpoint's model_state_dict of another, differently seeded policy (its actor is all the option reads)."""
    g = torch.Generator().manual_seed(seed)
    dims, sd = [no] + list(hidden) + [A], {"std": torch.ones(A)}
    for l in range(len(dims) - 1):
        bound = 1.0 / np.sqrt(dims[l])
        sd["actor.%d.weight" % (2 * l)] = (torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound
        sd["actor.%d.bias" % (2 * l)] = (torch.rand(dims[l + 1], generator=g) * 2 - 1) * bound
    return sd


def _runner(tmp=None, guide=None, seed=31, exact=False, save_interval=50, combined=False, fixed_lr=False):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if fixed_lr:
        train_cfg.algorithm.schedule = "fixed"
    if guide is not None:
        train_cfg.algorithm.guidance_cfg = guide
    if combined:
        train_cfg.algorithm.rnd_cfg = dict(weight=0.5, predictor_hidden_dims=[256, 128, 128], target_hidden_dims=[256, 128, 128])
        train_cfg.algorithm.value_normalization = True
        train_cfg.policy.empirical_normalization = True
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert PPO.guidance is None
    return runner


def _state(runner):
    torch.cuda.synchronize()
    net, st = runner.alg.net, runner.alg.storage
    return [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all[0].clone()]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _learn_logged(r, iterations):
    """learn() one iteration at a time -> the option's log ({loss, coef}) and its graph-key entry behind every iteration."""
    out = []
    for i in range(iterations):
        r.learn(num_learning_iterations=1, init_at_random_ep_len=(i == 0))
        torch.cuda.synchronize()
        g = r.alg._guide
        out.append((dict(g.read_log(r.alg._log.split(r.alg.log_block().cpu()))), dict(r.alg.update_graph_key())["guidance"]))
    return out


@pytest.mark.parametrize("plan", list(PLANS))
def test_captured_equals_eager_across_the_run_out(monkeypatch, plan):
    from humanoid.algo.ppo import guidance as GD
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    cfg = dict(LINEAR, teacher=_teacher())
    a = _runner(guide=cfg)
    assert a.alg._guide is not None and a.alg._guide.active and a.alg._options[-1] is a.alg._guide and a.alg._scalar_order[-1] is a.alg._guide
    a.learn(num_learning_iterations=6, init_at_random_ep_len=True)
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(guide=cfg)
    b.learn(num_learning_iterations=6, init_at_random_ep_len=True)
    assert b._update_graph is None
    assert _same(sa, _state(b)), "plan %s: the captured update and the eager one differ" % plan
    if plan == "default":
        assert a._update_graph is not None and a.alg.update_capturable()
    for r in (a, b):
        g = r.alg._guide
        assert g.count == 6 and not g.active and dict(r.alg.update_graph_key())["guidance"] == ("run out",)
        assert int(g.count_dev) == FINAL      # the device count stopped where the term left the update
        assert float(g.block.abs().sum()) == 0.0 and float(g.coef) == 0.0      # retired: the log reads 0
    # one iteration at a time, eager: the logged coefficient is the twin's at every update, the key changes once
    c = _runner(guide=cfg)
    log = _learn_logged(c, 5)
    s = GD.parse_schedule(LINEAR["coef"], LINEAR["coef_schedule"])
    for k, (entry, key) in enumerate(log):
        want = GD.schedule_coef(s, k) if k < FINAL else 0.0
        print("update %d: Guidance/coef %.6f (twin %.6f)  Loss/guidance %.5e  key %s" % (k, entry["coef"], want, entry["loss"], "run out" if key == ("run out",) else "on"))
        assert entry["coef"] == want
        assert (entry["loss"] > 0 and np.isfinite(entry["loss"])) if k < FINAL else entry["loss"] == 0.0
        assert (key == ("run out",)) == (k + 1 >= FINAL)
    assert c.alg.last_guidance == log[-1][0]
    assert dict(c.alg.log_scalars()) == {"Loss/guidance": 0.0, "Guidance/coef": 0.0}


def test_run_out_continues_as_an_unguided_run_and_resume_is_exact(tmp_path, monkeypatch):
    from humanoid.algo.ppo import checkpoint as CK
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = dict(LINEAR, teacher=_teacher())
    u = _runner(tmp_path / "u", guide=cfg, exact=True, save_interval=1)
    u.learn(num_learning_iterations=5, init_at_random_ep_len=True)
    u.wait_for_saves()
    final = _state(u)
    # every checkpoint carries the key (both save paths write the same dict): the count, the schedule, the teacher's tensors
    for it, count in ((1, 2), (2, 3), (5, 5)):
        ck = torch.load(os.path.join(u.log_dir, "model_%d.pt" % it), map_location="cpu")
        sd = ck[CK.GUIDE_KEY]
        assert list(ck)[:4] == ["model_state_dict", "optimizer_state_dict", "iter", "infos"] and list(ck)[-1] == CK.GUIDE_KEY
        assert sd["count"] == count and sd["schedule"] == u.alg._guide.schedule and sd["teacher_hidden_dims"] == [512, 256, 128]
        assert all(torch.equal(sd["teacher"][k], v) for k, v in _teacher().items() if k.startswith("actor."))
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")      # the blocking path writes the same entry
    u.save(str(tmp_path / "blocking.pt"))
    monkeypatch.delenv("HGYM_ASYNC_SAVE")
    blocking = torch.load(tmp_path / "blocking.pt", map_location="cpu")[CK.GUIDE_KEY]
    assert blocking["count"] == 5 and blocking["schedule"] == sd["schedule"] and all(torch.equal(blocking["teacher"][k], sd["teacher"][k]) for k in sd["teacher"])
    # an exact resume mid-schedule (two updates done, the third still guided), WITHOUT a teacher file
    r = _runner(tmp_path / "r", guide=dict(LINEAR, teacher=None, teacher_hidden_dims=[512, 256, 128]), exact=True)
    assert not r.alg._guide.loaded
    with pytest.raises(RuntimeError, match="teacher is not loaded"):
        r.alg._guide.teacher_pass(r.alg.storage)
    r.load(os.path.join(u.log_dir, "model_1.pt"))
    assert r.current_learning_iteration == 2 and r.alg._guide.count == 2 and r.alg._guide.loaded and r.alg._guide.active
    r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(final, _state(r)), "the resumed run left the uninterrupted one"
    # after the run-out (three updates done) an UNGUIDED run continues to the same bits: the checkpoint minus its guidance entry
    ck = torch.load(os.path.join(u.log_dir, "model_2.pt"), map_location="cpu")
    assert ck.pop(CK.GUIDE_KEY)["count"] == FINAL
    os.makedirs(tmp_path / "plain", exist_ok=True)
    torch.save(ck, tmp_path / "plain" / "model_2.pt")
    torch.save(torch.load(CK.env_state_path(os.path.join(u.log_dir, "model_2.pt")), map_location="cpu"), tmp_path / "plain" / "envstate_2.pt")
    p = _runner(tmp_path / "p", exact=True)
    assert p.alg._guide is None
    p.load(str(tmp_path / "plain" / "model_2.pt"))
    assert p.current_learning_iteration == 3
    p.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    p.wait_for_saves()
    assert _same(final, _state(p)), "after the run-out the guided run is not the unguided continuation"
    # load() refuses by key name: with the key for a run without, the reverse, another schedule
    with pytest.raises(RuntimeError, match="carries `guidance_state_dict`"):
        p.load(os.path.join(u.log_dir, "model_2.pt"))
    with pytest.raises(RuntimeError, match="has no `guidance_state_dict`"):
        r.load(str(tmp_path / "plain" / "model_2.pt"))
    other = _runner(guide=dict(LINEAR, coef=1.0, teacher=_teacher()))
    with pytest.raises(RuntimeError, match="schedule"):
        other.load(os.path.join(u.log_dir, "model_2.pt"))


def test_off_means_absent_and_the_parents_launches(monkeypatch, tmp_path):
    r = _runner()
    alg = r.alg
    key = alg.update_graph_key()
    assert alg._guide is None and alg.guidance is None and alg._options == () and dict(key)["guidance"] is None and key[-1] == ("guidance", None)
    assert alg.log_block().numel() == alg.net.opt_state.numel() == L.OPT_STATE and list(alg._log.split(alg.log_block().cpu())) == ["opt"]
    assert not hasattr(alg.storage, "teacher_mu") and alg.last_guidance is None and alg.log_scalars() == []
    calls = []
    monkeypatch.setattr(alg.net, "ppo_grad_guide", lambda *a: calls.append("guide"))
    grad = alg.net.ppo_grad
    monkeypatch.setattr(alg.net, "ppo_grad", lambda *a: (calls.append("plain"), grad(*a)))
    import hgym
    monkeypatch.setattr(hgym, "guide_schedule", lambda *a: calls.append("schedule"))
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert calls == ["plain"] * (2 * 2 * 2)      # iterations x epochs x minibatches, nothing else
    monkeypatch.undo()
    # ... an explicit None, and a schedule that is 0 everywhere, are the same run, bit for bit, with the same key and the same log block
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    for cfg in (None, dict(teacher=_teacher(), coef=0.0), dict(teacher=_teacher(), coef=0.0, coef_schedule=dict(mode="step", final_step=2, final_value=0.0))):
        q = _runner(guide=cfg)
        assert q.alg._guide is None and [n for n, _ in q.alg.update_graph_key()] == [n for n, _ in key] and q.alg.log_block().numel() == L.OPT_STATE
        q.learn(num_learning_iterations=2, init_at_random_ep_len=True)
        assert _same(_state(r), _state(q))
    for async_save in ("1", "0"):      # both save paths: the reference's four keys and nothing else
        monkeypatch.setenv("HGYM_ASYNC_SAVE", async_save)
        r.save(str(tmp_path / ("off%s.pt" % async_save)))
        assert list(torch.load(tmp_path / ("off%s.pt" % async_save), map_location="cpu")) == ["model_state_dict", "optimizer_state_dict", "iter", "infos"]


def test_everything_else_on(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = dict(LINEAR, teacher=_teacher())
    a = _runner(guide=cfg, combined=True)
    alg = a.alg
    assert alg._rnd is not None and alg._obs_norm is not None and alg.value_normalizer is not None and alg._guide is not None
    a.learn(num_learning_iterations=5, init_at_random_ep_len=True)
    sa = _state(a)
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _runner(guide=cfg, combined=True)
    logs = _learn_logged(b, 5)
    assert _same(sa, _state(b))
    assert all(torch.isfinite(t.double()).all() for t in sa)
    assert [e["coef"] > 0 for e, _ in logs] == [True] * FINAL + [False] * (5 - FINAL) and all(e["loss"] > 0 for e, _ in logs[:FINAL])
    block = b.alg.log_block().cpu()
    parts = b.alg._log.split(block)
    assert list(parts)[-2:] == ["guide", "guide_coef"] and b.alg._rnd.read_log(parts)["Loss/rnd"] > 0      # every tail is read where it lies
    assert block.numel() == L.OPT_STATE + b.alg._rnd.LOG_DOUBLES + 3 + 3


def test_teacher_pass_in_ragged_pieces_equals_one_forward():
    """teacher_max_batch = 200: the 512 stored rows go through in pieces of 192, 192 and 128 rows; a teacher with room for all of them
    gives the same bits in one hgym_mlp_forward."""
    small = _runner(guide=dict(coef=1.0, teacher=_teacher(), teacher_max_batch=200))
    whole = _runner(guide=dict(coef=1.0, teacher=_teacher(), teacher_max_batch=N * T))
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = torch.randn(T + 1, N, 705, device="cuda", generator=g)
    outs = []
    for r in (small, whole):
        st = r.alg.storage
        with torch.inference_mode():
            st._obs_all.copy_(rows)
            st.teacher_mu.fill_(float("nan"))
            r.alg._guide.teacher_pass(st)
        torch.cuda.synchronize()
        assert torch.isfinite(st.teacher_mu[:T]).all() and torch.isnan(st.teacher_mu[T]).all()      # the T N stored rows, never slot T
        outs.append(st.teacher_mu[:T].clone())
    assert int(small.alg._guide.tnet.cfg.max_batch) == 200 and int(whole.alg._guide.tnet.cfg.max_batch) == N * T
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    one = whole.alg._guide.tnet.forward(0, rows[:T].flatten(0, 1).contiguous())
    assert torch.equal(one.view(torch.int32), outs[1].flatten(0, 1).view(torch.int32))
    assert float(outs[0].abs().max()) > 0.0


def test_guided_run_approaches_the_teacher(monkeypatch):
    """A constant coefficient of 50 (the term outweighs the surrogate), a fixed learning rate: over ten updates the MSE between the
    student's and the teacher's means on 64 fixed rows -- the env's first observations -- falls, and ends below the same run unguided."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    g = _runner(guide=dict(coef=50.0, teacher=_teacher()), fixed_lr=True)
    p = _runner(fixed_lr=True)
    rows = g.env.get_observations().clone()
    assert torch.equal(rows, p.env.get_observations())
    with torch.inference_mode():
        t = g.alg._guide.tnet.forward(0, rows).clone()
    mse = lambda r: float(((r.alg.net.forward(0, rows) - t) ** 2).mean())
    with torch.inference_mode():
        before = mse(g)
        assert before == mse(p) and before > 0
    g.learn(num_learning_iterations=10, init_at_random_ep_len=True)
    p.learn(num_learning_iterations=10, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    with torch.inference_mode():
        guided, plain = mse(g), mse(p)
    print("MSE to the teacher on 64 fixed rows: %.5e before, %.5e after ten guided updates, %.5e after ten unguided" % (before, guided, plain))
    assert guided < before and guided < plain
    assert g.alg._guide.active and g.alg._guide.count == 10 and int(g.alg._guide.count_dev) == 10      # a constant schedule never runs out


def test_init_storage_refusals():
    from humanoid.algo import PPO
    from humanoid.utils.symmetry import xbot_l_mirror
    r = _runner()
    ac = r.alg.actor_critic
    alg = PPO(ac, num_mini_batches=2, device=r.device)
    alg.guidance = dict(coef=1.0, teacher=_teacher())
    alg.symmetry = xbot_l_mirror(r.env.cfg)
    with pytest.raises(ValueError, match="PPO.guidance does not support PPO.symmetry"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.symmetry_augmentation, alg.mirror_loss_coef = False, 0.5
    with pytest.raises(ValueError, match="PPO.guidance does not support PPO.symmetry"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.symmetry, alg.mirror_loss_coef = None, 0.0
    alg.smoothness = dict(temporal_coef=1.0)
    with pytest.raises(ValueError, match="PPO.guidance does not support PPO.smoothness"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.smoothness = None
    alg.guidance = dict(coef=1.0, teacher=_teacher(no=700))
    with pytest.raises(ValueError, match="num_actor_obs is 705"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.guidance = dict(coef=1.0, teacher=_teacher(A=10))
    with pytest.raises(ValueError, match="num_actions is 12"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.guidance = dict(coef=1.0)
    with pytest.raises(ValueError, match="teacher_hidden_dims is needed"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.guidance = dict(coeff=1.0)
    with pytest.raises(ValueError, match="unknown key coeff"):
        alg.init_storage(N, T, [705], [219], [12])
    alg.guidance = dict(coef=1.0, teacher=_teacher())
    alg._world = 2
    with pytest.raises(ValueError, match="one rank"):
        alg.init_storage(N, T, [705], [219], [12])
    from humanoid.algo.ppo.distillation import Distillation
    assert issubclass(Distillation, PPO)
