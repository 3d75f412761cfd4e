"""CPU: OnPolicyRunner's loop plan (_plan_loop) against a restatement of the expressions learn() evaluated inline before the plan
existed, over every HGYM_* loop knob, logging on / off, each native extension of the env and the algorithm, and each fused-rollout
mode; building a plan binds nothing."""
import dataclasses
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

from humanoid.algo.ppo.on_policy_runner import _plan_loop
from humanoid.algo.ppo.ppo import PPO

KNOBS = ("HGYM_GRAPH", "HGYM_ENV_SINK", "HGYM_LOG_SINK", "HGYM_DEFER_FIN", "HGYM_FUSE_ROLLOUT", "HGYM_ASYNC", "HGYM_GRAPH_UPDATE")
# env native extensions the plan looks for (log_sink_supported comes with bind_log_sink)
CAPS = ("bind_outputs", "bind_transition", "bind_log_sink", "take_pending_finalize", "rollout_fused_mode")
KINDS = ("ppo", "ppo_nodeferred", "plain")


class _Env:
    def __init__(self, priv=True, send_timeouts=True, supported=True, fused=None):
        self.cfg = SimpleNamespace(env=SimpleNamespace(send_timeouts=send_timeouts))
        self._priv, self._supported, self._fused, self.calls = priv, supported, fused, []

    def get_privileged_observations(self):
        return torch.zeros(1) if self._priv else None


def _env_class(caps):
    methods = dict(
        bind_outputs=lambda self, obs, priv: self.calls.append("bind_outputs"),
        bind_transition=lambda self, sink, defer_finalize=False: self.calls.append("bind_transition"),
        take_pending_finalize=lambda self: None,
        rollout_fused_mode=lambda self, net: self._fused)
    if "bind_log_sink" in caps:
        methods.update(bind_log_sink=lambda self, on: self.calls.append("bind_log_sink") or self._supported,
                       log_sink_supported=lambda self: self._supported)
    return type("Env_" + "_".join(caps), (_Env,), {k: v for k, v in methods.items() if k in caps or k == "log_sink_supported"})


class _StubPPO(PPO):
    """A PPO made without __init__: only what the plan reads."""

    def update_capturable(self):
        return self._capturable


class _Absent:
    """A class attribute that reads as missing: hasattr() is False on the instances."""

    def __get__(self, obj, cls):
        raise AttributeError


class _StubPPONoDeferred(_StubPPO):
    """A PPO whose class has no deferred_values: the plan runs a "deferred" fused mode as "inline"."""
    deferred_values = _Absent()


class _PlainAlg:
    """An algorithm without the native extensions PPO adds (but with a storage that has slots)."""

    def transition_sink(self):
        return None

    def update_capturable(self):
        return True


def _alg(kind, slots=True, capturable=True):
    a = object.__new__(dict(ppo=_StubPPO, ppo_nodeferred=_StubPPONoDeferred, plain=_PlainAlg)[kind])
    a.storage = SimpleNamespace(_obs_all=torch.zeros(2), _priv_all=torch.zeros(2)) if slots else SimpleNamespace()
    a.net, a._capturable = object(), capturable
    return a


def _today(env, alg, device, log_on):
    """learn()'s inline expressions before the loop plan (bind_log_sink(True) returned exactly what log_sink_supported() returns)."""
    e = lambda k: os.environ.get(k, "1") != "0"
    st = alg.storage
    obs_all, priv_all = getattr(st, "_obs_all", None), getattr(st, "_priv_all", None)
    privileged_obs = env.get_privileged_observations()
    zero_copy = obs_all is not None and priv_all is not None and hasattr(env, "bind_outputs") and privileged_obs is not None
    use_graph = (zero_copy and str(device).startswith("cuda") and os.environ.get("HGYM_GRAPH", "1") != "0" and hasattr(torch.cuda, "CUDAGraph"))
    sink_ok = (zero_copy and hasattr(env, "bind_transition") and hasattr(alg, "transition_sink")
               and getattr(env.cfg.env, "send_timeouts", False) and e("HGYM_ENV_SINK"))
    log_sink = bool(log_on and sink_ok and hasattr(env, "bind_log_sink") and e("HGYM_LOG_SINK") and env.log_sink_supported())
    host_log = log_on and not log_sink
    defer_ok = (sink_ok and not host_log and hasattr(env, "take_pending_finalize") and isinstance(alg, PPO) and e("HGYM_DEFER_FIN"))
    fuse_mode = (env.rollout_fused_mode(alg.net) if (defer_ok and hasattr(env, "rollout_fused_mode") and hasattr(alg, "fused_rollout_step")
                                                     and e("HGYM_FUSE_ROLLOUT")) else None)
    deferred = fuse_mode == "deferred" and hasattr(alg, "deferred_values")
    async_iters = (not log_on) and str(device).startswith("cuda") and isinstance(alg, PPO) and e("HGYM_ASYNC")
    async_log = log_sink and str(device).startswith("cuda") and isinstance(alg, PPO) and e("HGYM_ASYNC")
    graph_update = bool(use_graph and (async_iters or async_log) and hasattr(alg, "update_capturable") and alg.update_capturable()
                        and e("HGYM_GRAPH_UPDATE"))
    return dict(zero_copy=bool(zero_copy), graph=bool(use_graph), env_sink=bool(sink_ok), log_sink=log_sink, defer_fin=bool(defer_ok),
                fuse=None if fuse_mode is None else "deferred" if deferred else "inline",
                async_mode="events" if async_iters else "log" if async_log else None, graph_update=graph_update)


def _check(env, alg, device, log_on):
    plan = _plan_loop(env, alg, device, log_on)
    assert dataclasses.asdict(plan) == _today(env, alg, device, log_on), (type(env).__name__, type(alg).__name__, log_on)
    assert env.calls == []          # planning binds nothing
    return plan


@pytest.mark.parametrize("knobs", list(itertools.product("01", repeat=len(KNOBS))), ids="".join)
def test_plan_equals_the_inline_expressions(monkeypatch, knobs):
    for k, v in zip(KNOBS, knobs):
        monkeypatch.setenv(k, v)
    for n in range(len(CAPS) + 1):
        for caps in itertools.combinations(CAPS, n):
            cls = _env_class(caps)
            for fused, log_on, kind in itertools.product((None, "inline", "deferred"), (False, True), KINDS):
                _check(cls(fused=fused), _alg(kind), "cuda:0", log_on)


def test_plan_conditions_outside_the_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cls = _env_class(CAPS)
    seen = set()
    for device, priv, send_timeouts, supported, slots, capturable, fused, log_on, kind in itertools.product(
            ("cuda:0", "cpu"), (True, False), (True, False), (True, False), (True, False), (True, False),
            (None, "inline", "deferred"), (False, True), KINDS):
        env = cls(priv=priv, send_timeouts=send_timeouts, supported=supported, fused=fused)
        seen.add(_check(env, _alg(kind, slots, capturable), device, log_on))
    # every field takes each of its values somewhere
    for f in dataclasses.fields(next(iter(seen))):
        values = {getattr(p, f.name) for p in seen}
        assert values == ({True, False} if f.type is bool else {None, "inline", "deferred"} if f.name == "fuse" else {None, "events", "log"})


def test_plain_env_and_algorithm_take_the_plain_path(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    plan = _check(_env_class(())(), _alg("plain", slots=False), "cuda:0", False)
    assert not (plan.zero_copy or plan.graph or plan.env_sink or plan.log_sink or plan.defer_fin or plan.graph_update)
    assert plan.fuse is None and plan.async_mode is None


def test_deferred_mode_without_deferred_values_runs_inline(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    env = _env_class(CAPS)(fused="deferred")
    assert _check(env, _alg("ppo"), "cuda:0", False).fuse == "deferred"
    assert not hasattr(_alg("ppo_nodeferred"), "deferred_values")
    assert _check(env, _alg("ppo_nodeferred"), "cuda:0", False).fuse == "inline"
