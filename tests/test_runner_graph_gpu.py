"""-m gpu: a replayed HIP graph leaves the host exactly where the eager launches leave it.  What compute_returns(), update() and a fused
rollout change on the host is written once (PPO._returns_done / _update_done / _rollout_done) and run behind the launches whether they were
issued, captured or replayed (PPO.after_rollout_replay / after_update_replay only call them): each must have run once per iteration under
every launch mechanism.  The stepwise rollout reaches its end state call by call, so every plain host attribute of the algorithm and its
rollout storage is also compared across the launch mechanisms, for each form of the rollout, after every rollout (before compute_returns)
and after every learn() call; and the update graph's key covers what update() bakes into its launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLAIN = (int, float, bool, str, type(None))
SKIP = {}       # attribute name -> why it may differ between launch mechanisms (none today)


def _runner(num_envs, seed):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    task_registry.train_cfgs[args.task].seed = seed
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


def _snapshot(obj):
    plain = lambda v: isinstance(v, PLAIN) or (isinstance(v, (list, tuple)) and all(isinstance(x, PLAIN) for x in v))
    # (lists are copied: the storage updates shadow_valid in place)
    return {k: (type(v).__name__, list(v) if isinstance(v, list) else v) for k, v in vars(obj).items() if plain(v) and k not in SKIP}


@pytest.mark.parametrize("rollout", ["inline", "deferred", "stepwise"])
def test_replayed_graphs_leave_the_eager_host_state(monkeypatch, rollout):
    from humanoid.algo import PPO
    PPO.precision = "bf16"
    monkeypatch.setenv("HGYM_ROLLOUT_CRITIC", "deferred" if rollout == "deferred" else "auto")
    monkeypatch.setenv("HGYM_FUSE_ROLLOUT", "0" if rollout == "stepwise" else "1")
    snaps = {}
    for graph, graph_update in (("1", "1"), ("1", "0"), ("0", "0"), ("0", "1")):
        monkeypatch.setenv("HGYM_GRAPH", graph)
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", graph_update)
        torch.manual_seed(2468)
        np.random.seed(2468)
        r = _runner(256, 79)
        alg = r.alg
        if rollout != "stepwise":
            assert r.env.rollout_fused_mode(alg.net) == rollout
        r.env.episode_length_buf = torch.arange(256, device="cuda") * 7
        got, calls = [], {}
        shared = ("_returns_done", "_update_done") + (("_rollout_done",) if rollout != "stepwise" else ())
        for name in shared:
            def counted(*a, _name=name, _inner=getattr(alg, name), **k):
                calls[_name] = calls.get(_name, 0) + 1
                return _inner(*a, **k)
            setattr(alg, name, counted)
        learn_step = r._learn_step

        def after_rollout(*a, **k):         # (learn() calls it right after the rollout: eager, captured or replayed)
            got.append(("after rollout", _snapshot(alg), _snapshot(alg.storage)))
            return learn_step(*a, **k)
        r._learn_step = after_rollout
        for n in (5, 2):
            r.learn(num_learning_iterations=n, init_at_random_ep_len=False)
            torch.cuda.synchronize()
            got.append(("after learn()", _snapshot(alg), _snapshot(alg.storage)))
        assert len(got) == 9
        # one definition of the host book-keeping behind eager, capturing and replaying iterations: once per iteration each
        assert calls == dict.fromkeys(shared, 7), (graph, graph_update, calls)
        assert (r._graph is not None) == (graph == "1")
        assert (r._update_graph is not None) == (graph == "1" and graph_update == "1")
        snaps[(graph, graph_update)] = got
        del r, alg
    ref = snaps[("0", "0")]
    T = ref[0][2]["num_transitions_per_env"][1]
    # the states the mirrors must reproduce: a full storage after each rollout, an empty one after each update
    assert [w for w, _, _ in ref] == ["after rollout"] * 5 + ["after learn()"] + ["after rollout"] * 2 + ["after learn()"]
    assert all(st["step"] == ("int", T) and st["shadow_valid"] == ("list", [True] * T) for w, _, st in ref if w == "after rollout")
    assert all(a["_deferred_ready"] == ("bool", rollout == "deferred") for w, a, _ in ref if w == "after rollout")
    assert ref[-1][1]["_perm_draws"] == ("int", 7) and ref[-1][2]["step"] == ("int", 0)
    for mode, got in snaps.items():
        for i, ((when, a_alg, a_st), (_, b_alg, b_st)) in enumerate(zip(got, ref)):
            diff = lambda a, b: {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)}
            assert a_alg == b_alg, (mode, i, when, diff(a_alg, b_alg))
            assert a_st == b_st, (mode, i, when, diff(a_st, b_st))


def test_update_graph_key_covers_shadows_comm_flip_and_world():
    from humanoid.algo import PPO
    PPO.precision = "bf16"
    alg = _runner(256, 80).alg
    key = alg.update_graph_key()
    st = alg.storage
    assert st._obs_bf16 is not None
    for name, obj, value in (("_obs_bf16", st, None), ("comm_flip", alg, True), ("_world", alg, alg._world + 1)):
        keep = getattr(obj, name)
        setattr(obj, name, value)
        assert alg.update_graph_key() != key, name
        setattr(obj, name, keep)
        assert alg.update_graph_key() == key, name
