"""-m gpu: critic-only training through the drop-in stack, at 64 envs, rollouts of 8 steps, 3 iterations.

Distillation.train_critic (gradient_length 4):
  * on against off: the student's parameters, sigma and every stored action are the same bits; the critic moves only with the option on;
    Loss/value_function is finite and positive; student_state_dict() loads into a PPO runner with the trained critic's tensors
  * storage.returns is what PPO.compute_returns gives on a clone of the same storage
PPO.critic_warmup_updates = 2 (2 minibatches x 2 epochs):
  * actor, std, their Adam moments and the learning rate keep their bits through two updates while the critic moves; the graph key's
    entry and the logged count follow
  * captured against eager is bit-equal across the switch, on the default and the stepwise plan
  * a run saved during warm-up and resumed exactly continues to the same bits; both save paths carry the key; load() refuses by key name
  * with the count at 0 the graph key, the log block and the checkpoint are the parent's
  * init_storage's refusal on several ranks, the optimiser state's on non-zero actor moments"""
import copy
import os

import numpy as np
import pytest
import torch

from hgym import _lib as L
import test_distillation_gpu as TD
from test_distillation_gpu import teacher_ckpt      # noqa: F401  (the module's fixture: a random-weight teacher saved through a PPO runner)

pytestmark = pytest.mark.gpu
N, T, ITS = 64, 8, 3
KNOBS = ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK", "HGYM_ASYNC_SAVE")
WIDE = TD.WIDE


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield
    from humanoid.algo import PPO
    PPO.precision = "bf16"


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ Distillation.train_critic
def _distill(teacher, tmp, train_critic, student=WIDE, **alg_kw):
    kw = dict(train_critic=True, **alg_kw) if train_critic else dict(alg_kw)
    r = TD._runner("humanoid_distill", tmp, student_hidden_dims=student, **kw)
    r.load(teacher)
    r.writer = rec = TD._Scalars()
    os.makedirs(r.log_dir, exist_ok=True)
    return r, rec


@pytest.mark.parametrize("fuse", ["1", "0"], ids=["one-launch", "stepwise"])
def test_train_critic_leaves_the_student_as_it_was(teacher_ckpt, tmp_path, monkeypatch, fuse):
    from humanoid.algo import Distillation
    monkeypatch.setenv("HGYM_FUSE_ROLLOUT", fuse)
    path, _ = teacher_ckpt
    # (one runner at a time: building a runner seeds torch's generator, which learn() draws the first episode lengths from)
    on, rec_on = _distill(path, tmp_path / "on", True, value_loss_coef=0.5, clip_param=0.3, gamma=0.99, lam=0.9)
    lo = on.alg.net.bucket_split
    params0, critic0 = on.alg.net.params.clone(), on.alg.net.params[lo:].clone()
    on.learn(num_learning_iterations=ITS, init_at_random_ep_len=True)
    on.wait_for_saves()
    off, rec_off = _distill(path, tmp_path / "off", False)
    assert _bits(params0, off.alg.net.params)
    off.learn(num_learning_iterations=ITS, init_at_random_ep_len=True)
    off.wait_for_saves()
    assert isinstance(on.alg, Distillation) and on.alg.train_critic is True and off.alg.train_critic is False and Distillation.train_critic is False
    assert (on.alg.value_loss_coef, on.alg.clip_param, on.alg.gamma, on.alg.lam) == (0.5, 0.3, 0.99, 0.9)
    assert (on.alg._vf_cfg.value_coef, on.alg._vf_cfg.unclipped) == (0.5, 0) and abs(on.alg._vf_cfg.clip_param - 0.3) < 1e-7
    assert on.alg.log_block().numel() == L.OPT_STATE + 4 and off.alg.log_block().numel() == L.OPT_STATE + 2
    assert list(on.alg._log.split(on.alg.log_block().cpu())) == ["opt", "bc", "vf"]
    torch.cuda.synchronize()
    a, b = on.alg, off.alg
    assert _bits(a.net.params[:lo], b.net.params[:lo]), "the student or std differs between train_critic on and off"
    assert _bits(a.net.sigma, b.net.sigma) and _bits(a.net.adam_m[:lo], b.net.adam_m[:lo]) and _bits(a.net.adam_v[:lo], b.net.adam_v[:lo])
    for col in ("actions", "mu", "sigma", "actions_log_prob", "dones"):      # (not the rewards: their time-out bootstrap adds gamma V)
        assert _bits(getattr(a.storage, col), getattr(b.storage, col)), "stored %s differ" % col
    assert _bits(a.storage._obs_all, b.storage._obs_all) and _bits(a.storage.teacher_actions, b.storage.teacher_actions)
    assert not _bits(a.net.params[lo:], critic0), "the critic did not move with train_critic on"
    assert _bits(b.net.params[lo:], critic0), "the critic moved with train_critic off"
    assert torch.isfinite(a.net.params).all() and float(a.net.opt_state[L.OPT_STEP]) == ITS * 2
    assert rec_on.tags["Loss/behavior"] == rec_off.tags["Loss/behavior"] and len(rec_on.tags["Loss/behavior"]) == ITS
    vl = rec_on.tags["Loss/value_function"]
    print("Loss/value_function over %d iterations: %s" % (ITS, ", ".join("%.5g" % v for v in vl)))
    assert len(vl) == ITS and all(np.isfinite(vl)) and min(vl) > 0.0 and a.last_value_loss == vl[-1]
    assert set(rec_off.tags["Loss/value_function"]) == {0.0} and set(rec_on.tags["Loss/surrogate"]) == {0.0}
    # the checkpoint's format is what it was: the critic's tensors were always in it
    ck = torch.load(os.path.join(on.log_dir, "model_%d.pt" % ITS), map_location="cpu")
    assert list(ck) == list(torch.load(os.path.join(off.log_dir, "model_%d.pt" % ITS), map_location="cpu"))
    assert list(ck["model_state_dict"]) == list(a.actor_critic.state_dict())
    # the student's half of the checkpoint starts a PPO runner with the TRAINED critic
    p = TD._runner("humanoid_ppo", None, seed=32, actor_hidden_dims=WIDE)
    p.alg.actor_critic.load_state_dict(a.actor_critic.student_state_dict(), strict=True)
    assert p.alg.net.bucket_split == lo and _bits(p.alg.net.params, a.net.params) and not _bits(p.alg.net.params[lo:], critic0)


def test_returns_are_ppos_own(teacher_ckpt):
    """Distillation.compute_returns with train_critic against PPO.compute_returns on a clone of the same storage: the same weights, the
    same stored rewards, values and dones, the same bootstrap observation -- the same returns and advantages, bit for bit."""
    from humanoid.algo import PPO
    path, _ = teacher_ckpt
    d = TD._runner("humanoid_distill", None, student_hidden_dims=WIDE, train_critic=True, gamma=0.97, lam=0.9)
    d.load(path)
    p = TD._runner("humanoid_ppo", None, actor_hidden_dims=WIDE, gamma=0.97, lam=0.9)
    p.alg.actor_critic.load_state_dict(d.alg.actor_critic.student_state_dict(), strict=True)
    assert type(p.alg) is PPO and _bits(p.alg.net.params, d.alg.net.params)
    g = torch.Generator().manual_seed(8)
    sd, sp = d.alg.storage, p.alg.storage
    cols = dict(rewards=torch.randn(T, N, 1, generator=g), values=torch.randn(T, N, 1, generator=g),
                dones=(torch.rand(T, N, 1, generator=g) < 0.1).to(torch.uint8))
    obs, priv = torch.randn(T + 1, N, sd._obs_all.shape[-1], generator=g), torch.randn(T + 1, N, sd._priv_all.shape[-1], generator=g)
    with torch.inference_mode():
        for st in (sd, sp):
            for k, v in cols.items():
                getattr(st, k).copy_(v.to(getattr(st, k).dtype).to("cuda"))
            st._obs_all.copy_(obs.to("cuda"))
            st._priv_all.copy_(priv.to("cuda"))
            st.returns.fill_(float("nan"))
        last = priv[T].to("cuda").contiguous()
        d.alg.compute_returns(last)
        p.alg.compute_returns(last)
    torch.cuda.synchronize()
    assert torch.isfinite(sd.returns).all() and _bits(sd.returns, sp.returns) and _bits(sd.advantages, sp.advantages)
    assert torch.isfinite(sd.teacher_actions).all() and float(sd.teacher_actions.abs().max()) > 0.0      # and the teacher's pass ran behind it


# ------------------------------------------------------------------------------------------------ PPO.critic_warmup_updates
WARM = 2


def _ppo(tmp=None, warm=None, seed=31, exact=False, save_interval=50):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = T
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if warm is not None:
        train_cfg.algorithm.critic_warmup_updates = warm
    env, _ = task_registry.make_env(name="humanoid_ppo", args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name="humanoid_ppo", args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert PPO.critic_warmup_updates == 0
    return runner


def _state(runner):
    torch.cuda.synchronize()
    net, st = runner.alg.net, runner.alg.storage
    return [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all[0].clone()]


def _same(a, b):
    return len(a) == len(b) and all(_bits(x, y) for x, y in zip(a, b))


def test_warmup_moves_the_critic_alone(monkeypatch):
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    r = _ppo(warm=WARM)
    alg, net = r.alg, r.alg.net
    w = alg._warmup
    assert w is not None and w.active and alg._options == (w,) and alg._scalar_order == (w,) and alg.critic_warmup_updates == WARM
    assert alg.log_block().numel() == L.OPT_STATE + 3 and list(alg._log.split(alg.log_block().cpu()))[-1] == "critic_warmup"
    lo = net.bucket_split
    before = dict(params=net.params.clone(), sigma=net.sigma.clone(), lr=net.opt_state[L.OPT_LR].clone())
    calls = []
    grad, vf = net.ppo_grad, net.vf_grad
    monkeypatch.setattr(net, "ppo_grad", lambda *a: (calls.append("ppo"), grad(*a)))
    monkeypatch.setattr(net, "vf_grad", lambda *a: (calls.append("vf"), vf(*a)))
    log = []
    for i in range(WARM + 1):
        key = dict(alg.update_graph_key())["critic_warmup"]
        r.learn(num_learning_iterations=1, init_at_random_ep_len=(i == 0))
        torch.cuda.synchronize()
        o = alg.read_log(alg.log_block().cpu())
        log.append((key, dict(w.last), dict(alg.log_scalars()), o["mean_value_loss"], o["mean_surrogate_loss"]))
        if i == WARM - 1:      # behind the last critic-only update
            same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert same(net.params[:lo], before["params"][:lo]) and same(net.sigma, before["sigma"]), "std or the actor moved during warm-up"
            assert int(net.adam_m[:lo].view(torch.int32).abs().max()) == 0 and int(net.adam_v[:lo].view(torch.int32).abs().max()) == 0
            assert torch.equal(net.opt_state[L.OPT_LR], before["lr"]) and float(net.opt_state[L.OPT_STEP]) == WARM * 4
            assert not same(net.params[lo:], before["params"][lo:]), "the critic did not move"
            assert float(net.opt_state[L.OPT_MINIBATCHES]) == 0.0 and w.done == WARM and not w.active
    assert calls == ["vf"] * (WARM * 4) + ["ppo"] * 4      # updates x epochs x minibatches
    assert [k for k, *_ in log] == [True, True, False] and dict(alg.update_graph_key())["critic_warmup"] is False
    for i, (_, last, scalars, value_loss, surrogate) in enumerate(log):
        print("update %d: %s  value loss %.5g  surrogate %.5g" % (i, last, value_loss, surrogate))
        if i < WARM:
            assert last["trained"] and last["remaining"] == WARM - i and scalars["Policy/critic_warmup_remaining"] == float(WARM - i)
            assert value_loss == last["value_loss"] and np.isfinite(value_loss) and value_loss > 0.0 and surrogate == 0.0
        else:      # the plain update: the value loss is opt_state's again, the option logs nothing
            assert not last["trained"] and scalars == {} and np.isfinite(value_loss) and value_loss > 0.0 and surrogate != 0.0
    assert not torch.equal(net.params[12:lo], before["params"][12:lo]) and float(net.opt_state[L.OPT_STEP]) == (WARM + 1) * 4


@pytest.mark.parametrize("plan", ["default", "unfused"])
def test_captured_equals_eager_across_the_switch(monkeypatch, plan):
    if plan == "unfused":
        monkeypatch.setenv("HGYM_FUSE_ROLLOUT", "0")
    a = _ppo(warm=WARM)
    a.learn(num_learning_iterations=5, init_at_random_ep_len=True)
    sa = _state(a)
    if plan == "default":
        assert a._update_graph is not None and a.alg.update_capturable()
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    b = _ppo(warm=WARM)
    b.learn(num_learning_iterations=5, init_at_random_ep_len=True)
    assert b._update_graph is None
    assert _same(sa, _state(b)), "plan %s: the captured update and the eager one differ" % plan
    for r in (a, b):
        w = r.alg._warmup
        assert w.done == WARM and not w.active and float(w.block.abs().sum()) == 0.0      # retired: the log reads 0
    # after the switch the run makes a plain run's launches: from the same state a run without the option continues to the same bits
    assert all(torch.isfinite(t.double()).all() for t in sa)


def test_resume_during_warmup_is_exact_and_load_refuses_by_key_name(tmp_path, monkeypatch):
    from humanoid.algo.ppo import checkpoint as CK
    u = _ppo(tmp_path / "u", warm=WARM, exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    final = _state(u)
    for it, done in ((0, 1), (1, 2), (4, 2)):      # every checkpoint carries the key (model_0.pt: one update done, one to go)
        ck = torch.load(os.path.join(u.log_dir, "model_%d.pt" % it), map_location="cpu")
        assert list(ck)[:4] == ["model_state_dict", "optimizer_state_dict", "iter", "infos"] and list(ck)[-1] == CK.WARMUP_KEY
        assert ck[CK.WARMUP_KEY] == dict(done=done, updates=WARM)
    monkeypatch.setenv("HGYM_ASYNC_SAVE", "0")      # the blocking path writes the same entry
    u.save(str(tmp_path / "blocking.pt"))
    monkeypatch.delenv("HGYM_ASYNC_SAVE")
    assert torch.load(tmp_path / "blocking.pt", map_location="cpu")[CK.WARMUP_KEY] == dict(done=2, updates=WARM)
    r = _ppo(tmp_path / "r", warm=WARM, exact=True)
    r.load(os.path.join(u.log_dir, "model_0.pt"))
    assert r.current_learning_iteration == 1 and r.alg._warmup.done == 1 and r.alg._warmup.active
    r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(final, _state(r)), "the run resumed during warm-up left the uninterrupted one"
    plain = _ppo(tmp_path / "p")
    with pytest.raises(RuntimeError, match="carries `critic_warmup_state_dict`"):
        plain.load(os.path.join(u.log_dir, "model_1.pt"))
    plain.save(str(tmp_path / "plain.pt"))
    with pytest.raises(RuntimeError, match="has no `critic_warmup_state_dict`"):
        r.load(str(tmp_path / "plain.pt"))


def test_count_zero_is_the_parent(tmp_path, monkeypatch):
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "0")
    strip = lambda key: [(n, v) for n, v in key if n not in ("storage", "net")]      # (two runners: two storages, two nets)
    calls, keys, states = [], [], []
    for warm in (None, 0):      # (one runner at a time: building a runner seeds torch's generator, which learn() draws from)
        z = _ppo(warm=warm)
        alg = z.alg
        assert alg._warmup is None and alg._options == () and alg.log_block().numel() == L.OPT_STATE and alg.log_scalars() == []
        assert dict(alg.update_graph_key())["critic_warmup"] is False and alg.update_graph_key()[-1] == ("guidance", None)
        keys.append(strip(alg.update_graph_key()))
        monkeypatch.setattr(alg.net, "vf_grad", lambda *a: calls.append("vf"))
        z.learn(num_learning_iterations=2, init_at_random_ep_len=True)
        states.append(_state(z))
    assert keys[0] == keys[1] and _same(states[0], states[1]) and calls == []
    for async_save in ("1", "0"):      # both save paths: the reference's four keys and nothing else
        monkeypatch.setenv("HGYM_ASYNC_SAVE", async_save)
        z.save(str(tmp_path / ("off%s.pt" % async_save)))
        assert list(torch.load(tmp_path / ("off%s.pt" % async_save), map_location="cpu")) == ["model_state_dict", "optimizer_state_dict", "iter", "infos"]


def test_refusals():
    from humanoid.algo import PPO
    r = _ppo()
    alg = PPO(r.alg.actor_critic, num_mini_batches=2, device=r.device)
    alg.critic_warmup_updates, alg._world = 2, 2
    with pytest.raises(ValueError, match="PPO.critic_warmup_updates runs on one rank"):
        alg.init_storage(N, T, [705], [219], [12])
    alg._world, alg.critic_warmup_updates = 1, -1
    with pytest.raises(ValueError, match="integer >= 0"):
        alg.init_storage(N, T, [705], [219], [12])
    # an optimiser state with non-zero actor moments while critic-only updates remain: refused before anything is changed
    trained = _ppo()
    trained.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    sd = trained.alg.optimizer.state_dict()
    w = _ppo(warm=WARM)
    m0 = w.alg.net.adam_m.clone()
    with pytest.raises(ValueError, match="non-zero Adam moments"):
        w.alg.optimizer.load_state_dict(sd)
    assert torch.equal(w.alg.net.adam_m, m0) and float(w.alg.net.opt_state[L.OPT_STEP]) == 0.0
    w.alg._warmup.done = WARM      # none remains: the same state loads
    w.alg.optimizer.load_state_dict(sd)
    assert torch.equal(w.alg.net.adam_m, trained.alg.net.adam_m)
    from humanoid.algo import Distillation, StudentTeacher
    pol = StudentTeacher(705, 219, 12, student_hidden_dims=[256, 128, 128], teacher_hidden_dims=[256, 128, 128], critic_hidden_dims=[256, 128, 128])
    d = Distillation(pol, gradient_length=4, device="cuda:0")
    d.critic_warmup_updates = 1
    with pytest.raises(ValueError, match="does not support Distillation"):
        d.init_storage(N, T, [705], [219], [12])
