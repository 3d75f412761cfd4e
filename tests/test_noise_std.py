"""ActorCritic(noise_std_type=...) and HgymNetConfig.std_param, host side: the parameter's name, place and initial value, what the
constructor and make_net_config refuse, the field's mirror, and what hgym_net_sigma_offset answers without a device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hgym import _lib as L, make_net_config

XBOTL = (705, 219, 12, [512, 256, 128], [768, 256, 128])


def _ac(**kw):
    from humanoid.algo.ppo.actor_critic import ActorCritic
    return ActorCritic(705, 219, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128], **kw)


def _cfg(precision="bf16", **kw):
    return make_net_config(*XBOTL, precision, 256, **kw)


def test_log_policy_has_log_std_first_and_no_std():
    ac = _ac(init_noise_std=0.5, noise_std_type="log")
    keys = list(ac.state_dict())
    assert keys[:3] == ["log_std", "actor.0.weight", "actor.0.bias"] and "std" not in keys
    assert not hasattr(ac, "std")
    assert ac.noise_std_type == "log"
    assert torch.equal(ac.log_std.detach(), torch.log(0.5 * torch.ones(12)))
    assert float(ac.log_std[0]) == float(np.float32(math.log(0.5)))
    # unbound: exp of the parameter, within 1 ulp of 0.5 (spacing of fp32 at 0.5 is 2^-24 below, 2^-23 above: the smaller one)
    s = ac.noise_std
    assert s.shape == (12,) and s.dtype == torch.float32 and not s.requires_grad
    assert float((s.double() - 0.5).abs().max()) <= 2.0 ** -24


def test_default_policy_is_unchanged():
    ac = _ac(init_noise_std=0.5)
    assert list(ac.state_dict())[:2] == ["std", "actor.0.weight"]
    assert not hasattr(ac, "log_std") and ac.noise_std_type == "scalar"
    assert torch.equal(ac.std.detach(), 0.5 * torch.ones(12))
    assert torch.equal(ac.noise_std, ac.std.detach())
    assert list(_ac(noise_std_type="scalar").state_dict()) == list(_ac().state_dict())


def test_other_types_are_refused_by_name(capsys):
    with pytest.raises(ValueError, match="scalar.*log"):
        _ac(noise_std_type="softplus")
    assert "Actor MLP" not in capsys.readouterr().out        # refused before anything is built
    with pytest.raises(ValueError, match="scalar.*log"):
        _cfg(noise_std_type="softplus")
    with pytest.raises(ValueError):
        _cfg(noise_std_type=None)


def test_field_and_constants():
    assert (L.STD_SCALAR, L.STD_LOG) == (0, 1)
    # directly ahead of fused_activation, which stays the struct's last field
    assert [f[0] for f in L.NetConfig._fields_[-2:]] == ["std_param", "fused_activation"]
    assert C.sizeof(L.NetConfig) == int(L.lib.hgym_sizeof(b"HgymNetConfig"))
    lo = L.NetConfig.std_param.offset
    assert lo == C.sizeof(L.NetConfig) - 8 and L.NetConfig.fused_activation.offset == lo + 4
    assert _cfg().std_param == L.STD_SCALAR and _cfg(noise_std_type="scalar").std_param == L.STD_SCALAR
    assert _cfg(noise_std_type="log").std_param == L.STD_LOG
    # the default leaves the field zero, and the field is all the switch changes
    a, b = _cfg(), _cfg(noise_std_type="log")
    raw = lambda c: bytes(memoryview(c).cast("B"))
    assert raw(a)[lo:lo + 4] == bytes(4) and raw(b)[lo:lo + 4] == (1).to_bytes(4, "little")
    assert raw(a)[:lo] == raw(b)[:lo] and raw(a)[lo + 4:] == raw(b)[lo + 4:]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_sigma_offset(precision):
    scalar, log = _cfg(precision), _cfg(precision, noise_std_type="log")
    assert int(L.lib.hgym_net_sigma_offset(C.byref(scalar))) == -1
    off = int(L.lib.hgym_net_sigma_offset(C.byref(log)))
    total = int(L.lib.hgym_net_workspace_bytes(C.byref(log)))
    assert off >= 0 and off % 4 == 0 and off + 64 <= total
    # the block is the only thing the mode adds: every size of the scalar mode stays
    assert int(L.lib.hgym_net_workspace_bytes(C.byref(scalar))) <= off
    assert int(L.lib.hgym_net_param_count(C.byref(log))) == int(L.lib.hgym_net_param_count(C.byref(scalar)))


@pytest.mark.parametrize("bad", [2, -1, 255])
def test_other_values_of_the_field_are_refused(bad):
    cfg = _cfg()
    cfg.std_param = bad
    assert int(L.lib.hgym_net_param_count(C.byref(cfg))) == -1
    assert b"std_param" in L.lib.hgym_last_error()
    assert int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) < 0
    assert int(L.lib.hgym_net_sigma_offset(C.byref(cfg))) == -2
    assert b"std_param" in L.lib.hgym_last_error()
    # HGYM_E_BADARG itself, from a call that returns the code (no device work is reached: the configuration is checked first)
    net = L.Net()
    assert int(L.lib.hgym_net_sync_shadow(C.byref(cfg), C.byref(net), None)) == -1
    cfg.std_param = L.STD_LOG
    assert int(L.lib.hgym_net_param_count(C.byref(cfg))) > 0


def test_runner_reads_noise_std_and_falls_back_to_std():
    from types import SimpleNamespace
    from humanoid.algo.ppo.on_policy_runner import OnPolicyRunner
    log = _ac(init_noise_std=0.25, noise_std_type="log")
    assert abs(float(OnPolicyRunner._noise_std(log).mean()) - 0.25) <= 2.0 ** -25
    assert float(OnPolicyRunner._noise_std(_ac(init_noise_std=0.75)).mean()) == 0.75
    stand_in = SimpleNamespace(std=torch.full((12,), 2.0))
    assert float(OnPolicyRunner._noise_std(stand_in).mean()) == 2.0

