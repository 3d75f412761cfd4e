"""-m gpu: the two role layouts of the fused rollout launch (csrc/hgym_rollout.hip) compute the same bits.  The 64-row layout (default
where the 32-row tiles pair up) runs 64-row critic tiles next to side-job workgroups that form the next step's draws, the rows
after next and the actor's carried first layer; HGYM_RO_CRITIC64=0 keeps the 32-row critic tiles that carry those jobs
themselves.  Three learning iterations of 60 steps (eager, capture + replay, replay) from the same seeds, about 5 % of the envs
forced to time out inside the first rollout and 5 % inside the third: storage (fp32 rows, bf16 shadows, values, actions, log-probabilities, rewards, dones),
the env state and the parameters must be equal, the episode sink's means equal to float-atomic order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _runner(num_envs, seed):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    task_registry.train_cfgs[args.task].seed = seed
    env, _ = task_registry.make_env(name=args.task, args=args)
    runner, _ = task_registry.make_alg_runner(env=env, name=args.task, args=args, log_root=None)
    return runner


def _run(monkeypatch, num_envs, layout, kb0):
    from humanoid.algo import PPO
    PPO.precision = "bf16"
    monkeypatch.setenv("HGYM_RO_CRITIC64", layout)
    if kb0 is None:
        monkeypatch.delenv("HGYM_L0_KB0", raising=False)
    else:
        monkeypatch.setenv("HGYM_L0_KB0", kb0)
    torch.manual_seed(17)
    np.random.seed(17)
    r = _runner(num_envs, 23)
    env = r.env
    # episode lengths: most envs early in their episode, ~5 % time out inside the first rollout and ~5 % inside the third (the one the
    # storage holds at the end)
    g = torch.Generator().manual_seed(5)
    L = int(env.max_episode_length)
    el = torch.randint(0, L // 2, (num_envs,), generator=g)
    u = torch.rand(num_envs, generator=g)
    first, third = u < 0.05, (u >= 0.05) & (u < 0.10)
    el[first] = L - torch.randint(1, 60, (int(first.sum()),), generator=g)
    el[third] = L - torch.randint(121, 180, (int(third.sum()),), generator=g)
    env.episode_length_buf = el.to(env.device)
    r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
    torch.cuda.synchronize()
    st = r.alg.storage
    out = dict(params=r.alg.net.params, obs=st._obs_all, priv=st._priv_all, obs_sh=st._obs_bf16, priv_sh=st._priv_bf16, act=st.actions,
               mu=st.mu, sigma=st.sigma, logp=st.actions_log_prob, val=st.values, rew=st.rewards, dones=st.dones)
    for k, v in vars(env._buf).items():
        if torch.is_tensor(v) and v.is_cuda and k != "_l0_partial":     # (the carried sums themselves: kb0 of the 24 k-steps)
            out["env." + k] = v
    for k, v in env._buf.f.items():
        out["env.f." + k] = v
    for k, v in env.extras.get("episode", {}).items():
        if torch.is_tensor(v):
            out["episode." + k] = v
    out = {k: v.detach().clone() for k, v in out.items() if v is not None}
    out["resets"] = int(st.dones.sum())
    out["l0_used"] = env._buf._l0_partial is not None and bool((env._buf._l0_partial != 0).any())
    del r
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    assert a["resets"] == b["resets"]
    n = a["dones"].shape[1]
    assert n < 1024 or a["resets"] >= 0.03 * n      # the forced time-outs happened (too few envs below 1024 to bound it)
    assert a["l0_used"] and b["l0_used"]
    # the episode sink's means come from float atomics of every env workgroup (the finaliser's accumulators): their order, hence their
    # last bits, changes from run to run in either layout -- compared as everywhere else in the suite (tests/env_common.py)
    sink = lambda k: k == "env.extras_episode" or k.startswith("episode.")
    bad = ["%s (%d of %d differ)" % (k, int((a[k] != b[k]).sum()), a[k].numel()) for k in a
           if torch.is_tensor(a[k]) and not sink(k) and not torch.equal(a[k], b[k])]
    bad += [k for k in a if sink(k) and not torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-7)]
    assert not bad, bad
    assert torch.isfinite(a["params"]).all()


_REF = {}


@pytest.mark.parametrize("kb0", [None, "12", "16", "20"])
def test_critic64_layout_equals_32_row_layout_4096(monkeypatch, kb0):
    """4096 envs: the 64-row layout at its default split (20 k-steps carried) and at 12 / 16 / 20 against the 32-row layout at ITS
    default split (12) -- the carried sums follow the same fragments in the same k order for every split."""
    if "ref" not in _REF:
        _REF["ref"] = _run(monkeypatch, 4096, "0", None)
    _same(_run(monkeypatch, 4096, "1", kb0), _REF["ref"])


@pytest.mark.parametrize("num_envs", [96, 64])
def test_layout_falls_back_where_the_tiles_do_not_pair(monkeypatch, num_envs):
    """96 envs (3 tiles of 32: odd) and 64 envs (fewer than 128) take the 32-row layout whatever HGYM_RO_CRITIC64 says."""
    _same(_run(monkeypatch, num_envs, "1", None), _run(monkeypatch, num_envs, "0", None))
