"""HgymNetConfig.fused_activation, host side: the field and its mirrors, what the library accepts and refuses, how ActorCritic resolves
the keyword and HGYM_FUSED_ACT, and that the flag at 0 or with ELU(1) leaves the configuration struct as it was."""
import ctypes as C

import pytest
import torch.nn as nn

from hgym import _lib as L, make_net_config

ACTS = [nn.ELU(0.5), nn.SELU(), nn.ReLU(), nn.LeakyReLU(0.01), nn.Tanh(), nn.Sigmoid()]
IDS = ["elu0.5", "selu", "relu", "leaky0.01", "tanh", "sigmoid"]


def _cfg(activation=None, precision="bf16", **kw):
    return make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, 4096, activation=activation, **kw)


def _bytes(cfg):
    return bytes(memoryview(cfg).cast("B"))


def test_field_is_last_and_sizes_agree():
    assert L.NetConfig._fields_[-1][0] == "fused_activation"
    assert C.sizeof(L.NetConfig) == int(L.lib.hgym_sizeof(b"HgymNetConfig"))
    assert L.NetConfig.fused_activation.offset == C.sizeof(L.NetConfig) - 4


def test_make_net_config_sets_the_field():
    assert _cfg(nn.Tanh()).fused_activation == 0
    assert _cfg(nn.Tanh(), fused_activation=False).fused_activation == 0
    assert _cfg(nn.Tanh(), fused_activation=True).fused_activation == 1


@pytest.mark.parametrize("bad", [2, -1, 255])
def test_other_values_are_refused(bad):
    cfg = _cfg(nn.Tanh())
    cfg.fused_activation = bad
    assert int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) < 0
    assert b"fused_activation" in L.lib.hgym_last_error()
    assert int(L.lib.hgym_net_param_count(C.byref(cfg))) < 0
    cfg.fused_activation = 1
    assert int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) > 0


@pytest.mark.parametrize("act", ACTS, ids=IDS)
def test_flag_selects_the_fused_layout(act):
    """hgym_net_shadow_ld is the host-side sign of the fused layout: 768 / 256 columns with the flag, 0 without; the parameter count is the
    same on both layouts."""
    off, on = _cfg(act), _cfg(act, fused_activation=True)
    assert [int(L.lib.hgym_net_shadow_ld(C.byref(off), i)) for i in (0, 1)] == [0, 0]
    assert [int(L.lib.hgym_net_shadow_ld(C.byref(on), i)) for i in (0, 1)] == [768, 256]
    assert int(L.lib.hgym_net_param_count(C.byref(on))) == int(L.lib.hgym_net_param_count(C.byref(off))) == 926105
    # the fused layout of this net is ELU(1)'s, byte for byte
    assert int(L.lib.hgym_net_workspace_bytes(C.byref(on))) == int(L.lib.hgym_net_workspace_bytes(C.byref(_cfg())))


def test_flag_is_ignored_where_the_fused_path_is_refused(monkeypatch):
    act = nn.Tanh()
    for kw in (dict(precision="f32"), dict()):
        cfg = _cfg(act, fused_activation=True, **kw) if kw else make_net_config(705, 219, 12, [768, 256, 128], [768, 256, 128], "bf16", 4096,
                                                                               activation=act, fused_activation=True)
        ref = _cfg(act, **kw) if kw else make_net_config(705, 219, 12, [768, 256, 128], [768, 256, 128], "bf16", 4096, activation=act)
        assert int(L.lib.hgym_net_shadow_ld(C.byref(cfg), 0)) == 0
        assert int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) == int(L.lib.hgym_net_workspace_bytes(C.byref(ref)))
    monkeypatch.setenv("HGYM_NO_FUSED", "1")
    assert int(L.lib.hgym_net_shadow_ld(C.byref(_cfg(act, fused_activation=True)), 0)) == 0


def test_elu1_and_flag_off_leave_the_struct_as_it_was():
    """Apart from the new last field, the struct is today's: with the flag left at 0 for every activation, and with the flag set on an
    ELU(1) net -- whose layout and sizes the flag does not change either."""
    for act in [None, nn.ELU()] + ACTS:
        a, b = _cfg(act), _cfg(act, fused_activation=True)
        assert _bytes(a)[:-4] == _bytes(b)[:-4] and _bytes(a)[-4:] == bytes(4) and _bytes(b)[-4:] == (1).to_bytes(4, "little")
    a, b = _cfg(nn.ELU()), _cfg(nn.ELU(), fused_activation=True)
    for fn in (L.lib.hgym_net_workspace_bytes, L.lib.hgym_net_param_count):
        assert int(fn(C.byref(a))) == int(fn(C.byref(b)))
    assert int(L.lib.hgym_net_shadow_ld(C.byref(a), 0)) == int(L.lib.hgym_net_shadow_ld(C.byref(b), 0)) == 768


def test_actor_critic_keyword_and_environment(monkeypatch):
    from humanoid.algo.ppo.actor_critic import ActorCritic
    mk = lambda **kw: ActorCritic(705, 219, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128], activation=nn.ReLU(), **kw)
    monkeypatch.delenv("HGYM_FUSED_ACT", raising=False)
    assert mk().fused_activation is False and mk(fused_activation=None).fused_activation is False
    assert mk(fused_activation=True).fused_activation is True and mk(fused_activation=False).fused_activation is False
    monkeypatch.setenv("HGYM_FUSED_ACT", "1")
    assert mk().fused_activation is True and mk(fused_activation=False).fused_activation is False
    monkeypatch.setenv("HGYM_FUSED_ACT", "0")
    assert mk().fused_activation is False and mk(fused_activation=True).fused_activation is True
    monkeypatch.setenv("HGYM_FUSED_ACT", "yes")          # only "1" means on
    assert mk().fused_activation is False
