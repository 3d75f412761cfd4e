"""CPU side of OnPolicyRunner.evaluate: the new C-ABI symbols, LeggedRobot.eval_rollout_supported on fake objects, and the
evaluation accumulator's arithmetic (numpy float64 restatement, tests/evaluate_common.py) on a hand-made trace with known answers --
the trace the GPU kernel gets in tests/test_evaluate_gpu.py."""
import math
import os
import re
from types import SimpleNamespace

import pytest

import evaluate_common as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hgym_rollout_eval_step", "hgym_eval_reset", "hgym_eval_accumulate")


def test_new_symbols_in_header_exports_and_bindings():
    from hgym import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgym.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SYMBOLS and hasattr(L.lib, name), name
    # the block layout the bindings mirror
    d = {k: int(v) for k, v in re.findall(r"#define\s+HGYM_EVAL_([A-Z_]+)\s+(\d+)", hdr)}
    assert d["SUMS"] == L.EVAL_SUMS == EC.SUMS and d["ENVS_PER_PARTIAL"] == L.EVAL_ENVS_PER_PARTIAL
    for nm in ("STEPS", "ENV_STEPS", "LIN_ERR", "ANG_ERR", "REWARD", "EPISODES", "TIMEOUTS", "RETURN", "LENGTH", "TICKET", "TERMS"):
        assert d[nm] == getattr(L, "EVAL_" + nm) == getattr(EC, nm), nm
    assert L.eval_block_doubles(4096) == 32 * (1 + 16) + 24 * 4096 and L.eval_block_doubles(5) == 32 * 2 + 24 * 5
    # null arguments are refused, not launched
    assert L.lib.hgym_eval_reset(0, None, None) == -1
    assert L.lib.hgym_eval_accumulate(0, None, None, None, None, None, None, None, None, None) == -2
    assert L.lib.hgym_rollout_eval_step(None, None, None, None, None, None, None, None, None, None, 0, None) == -1


def _fake_env(**over):
    from humanoid.envs.base.legged_robot import LeggedRobot
    c = dict(custom_origins=0, terrain_curriculum=0, num_height_points=0, command_curriculum=0, heading_command=1, use_ref_actions=0,
             frame_stack=15, c_frame_stack=3)
    c.update({k: v for k, v in over.items() if k in c})
    env = object.__new__(LeggedRobot)
    env._ncfg = SimpleNamespace(**c)
    env._L = SimpleNamespace(BF16=1, lib=SimpleNamespace(hgym_device_cus=lambda: over.get("cus", 256)))
    env.num_envs = over.get("num_envs", 4096)
    env._custom_terms = over.get("custom_terms", [])
    env.cfg = SimpleNamespace(env=SimpleNamespace(send_timeouts=over.get("send_timeouts", True)))
    return env


def _fake_net(**over):
    cfg = dict(precision=1, actor_layers=4, critic_layers=4, actor_dims=[705, 512, 256, 128, 12], critic_dims=[219, 768, 256, 128, 1],
               num_actions=12, max_batch=61440)
    cfg.update({k: v for k, v in over.items() if k in cfg})
    return SimpleNamespace(cfg=SimpleNamespace(**cfg), shadow_ld=lambda which: over.get("shadow_ld", 768))


def test_eval_rollout_supported_rules():
    """The rules of rollout_fused_mode minus the critic, the storage and send_timeouts."""
    assert _fake_env().eval_rollout_supported(_fake_net())
    # what the training launch refuses but the evaluation launch does not care about
    assert _fake_env(send_timeouts=False).eval_rollout_supported(_fake_net())
    assert _fake_env().eval_rollout_supported(_fake_net(critic_layers=3, critic_dims=[219, 256, 256, 1]))
    assert _fake_env(num_envs=8192).eval_rollout_supported(_fake_net())          # one workgroup per 32 envs: a whole chip of envs
    assert _fake_env(num_envs=16384, cus=256).eval_rollout_supported(_fake_net())   # ... or more: the workgroups are independent
    assert not _fake_env(send_timeouts=False).rollout_fused_mode(_fake_net())
    # what both refuse
    for bad in (dict(num_envs=4097), dict(custom_origins=1), dict(terrain_curriculum=1), dict(num_height_points=9),
                dict(command_curriculum=1), dict(heading_command=0), dict(use_ref_actions=1), dict(frame_stack=5), dict(c_frame_stack=1),
                dict(custom_terms=[("x", None, 1.0)])):
        assert not _fake_env(**bad).eval_rollout_supported(_fake_net()), bad
    for bad in (dict(precision=0), dict(actor_layers=3), dict(actor_dims=[705, 256, 256, 128, 12]), dict(num_actions=10), dict(shadow_ld=0),
                dict(max_batch=2048)):
        assert not _fake_env().eval_rollout_supported(_fake_net(**bad)), bad
    # the training launch's own answer is what it was
    assert _fake_env().rollout_fused_mode(_fake_net()) == "inline" and _fake_env(num_envs=8192).rollout_fused_mode(_fake_net()) == "deferred"

    class Wrapped(type(_fake_env())):
        def step(self, actions):
            return super().step(actions)
    w = _fake_env()
    w.__class__ = Wrapped
    assert not w.eval_rollout_supported(_fake_net())           # a task class with its own step() keeps getting it


def test_accumulator_arithmetic_on_the_hand_made_trace():
    from humanoid.envs.base.legged_robot import KERNEL_REWARD_TERMS, eval_summary, EVAL_KEYS
    n, steps = EC.hand_trace()
    acc = EC.EvalAccumulatorNp(n)
    for s in steps:
        acc.add(**s)
    t = acc.totals
    assert t[EC.STEPS] == 3 and t[EC.ENV_STEPS] == 15 and t[EC.EPISODES] == 2 and t[EC.TIMEOUTS] == 1
    assert t[EC.LIN_ERR] == 15.0 and t[EC.ANG_ERR] == 3.75 and t[EC.REWARD] == 15.0 and t[EC.RETURN] == 4.5 and t[EC.LENGTH] == 5.0
    got = eval_summary(t.tolist(), KERNEL_REWARD_TERMS, 24.0)
    exp = EC.hand_trace_expected(KERNEL_REWARD_TERMS, 24.0)
    assert set(got) == set(exp) == set(EVAL_KEYS) | {"rew_" + k for k in KERNEL_REWARD_TERMS}
    for k in exp:
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert isinstance(got["episodes"], int) and all(isinstance(v, float) for k, v in got.items() if k != "episodes")


def test_no_finished_episode_gives_nan_episode_fields():
    from humanoid.envs.base.legged_robot import KERNEL_REWARD_TERMS, eval_summary
    n, steps = EC.hand_trace()
    acc = EC.EvalAccumulatorNp(n)
    acc.add(**steps[0])
    got = eval_summary(acc.totals.tolist(), KERNEL_REWARD_TERMS, 24.0)
    assert got["episodes"] == 0 and got["mean_reward_per_step"] == 0.5 and got["lin_vel_tracking_error"] == 1.0
    for k in ("mean_episode_return", "mean_episode_length", "timeout_fraction", "fall_fraction", "rew_torques"):
        assert math.isnan(got[k]), k
    # only the kernel's terms are reported
    assert "rew_mine" not in eval_summary(acc.totals.tolist(), ["torques", "mine"], 24.0)


def test_evaluate_refuses_the_training_env():
    from humanoid.algo.ppo.on_policy_runner import OnPolicyRunner
    r = object.__new__(OnPolicyRunner)
    r.env = object()
    with pytest.raises(ValueError):
        r.evaluate(r.env, 10)
    with pytest.raises(ValueError):
        r.set_eval_env(r.env)
