"""The hidden-layer activation as a configuration choice (HgymNetConfig.activation), host side: what ActorCritic accepts
and refuses, what make_net_config writes, what the library validates, and that a zero-filled tail is today's ELU(1) net."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from hgym import _lib as L, make_net_config, activation_spec

SUPPORTED = [
    (nn.ELU(), (L.ACT_ELU, 1.0, 1.0)),
    (nn.ELU(alpha=0.5), (L.ACT_ELU, 0.5, 1.0)),
    (nn.SELU(), (L.ACT_SELU, 1.6732632423543772, 1.0507009873554805)),
    (nn.ReLU(), (L.ACT_LEAKY_RELU, 0.0, 0.0)),
    (nn.LeakyReLU(0.01), (L.ACT_LEAKY_RELU, 0.01, 0.0)),
    (nn.Tanh(), (L.ACT_TANH, 0.0, 0.0)),
    (nn.Sigmoid(), (L.ACT_SIGMOID, 0.0, 0.0)),
]
IDS = ["elu", "elu0.5", "selu", "relu", "leaky0.01", "tanh", "sigmoid"]


class MyTanh(nn.Tanh):
    def forward(self, x):
        return 2.0 * torch.tanh(x)


UNSUPPORTED = [nn.GELU(), nn.LeakyReLU(-0.1), nn.ELU(alpha=-1.0), nn.Softplus(), MyTanh(), nn.Identity()]


def _cfg(activation=None, precision="bf16", **kw):
    return make_net_config(705, 219, 12, [512, 256, 128], [768, 256, 128], precision, 4096, activation=activation, **kw)


def _sizes(cfg):
    return int(L.lib.hgym_net_param_count(C.byref(cfg))), int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))


@pytest.mark.parametrize("module,spec", SUPPORTED, ids=IDS)
def test_actor_critic_accepts_and_keeps_the_module(module, spec):
    from humanoid.algo.ppo.actor_critic import ActorCritic
    ac = ActorCritic(705, 219, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128], activation=module,
                     denoiser_hidden_dims=[256, 128], denoiser_targets=9)
    for seq in (ac.actor, ac.critic, ac.denoiser):
        acts = [m for m in seq if not isinstance(m, nn.Linear)]
        assert len(acts) == len(seq) // 2 and all(m is module for m in acts)
    ref = ActorCritic(705, 219, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128])
    assert list(ac.state_dict()) == list(ref.state_dict()) + [k for k in ac.state_dict() if k.startswith("denoiser.")]
    assert sum(p.numel() for n, p in ac.named_parameters() if not n.startswith("denoiser.")) == 926105


@pytest.mark.parametrize("module", UNSUPPORTED, ids=lambda m: type(m).__name__ + str(getattr(m, "negative_slope", getattr(m, "alpha", ""))))
def test_unsupported_activations_still_raise(module):
    from humanoid.algo.ppo.actor_critic import ActorCritic
    with pytest.raises(NotImplementedError, match="supported: nn.ELU"):
        ActorCritic(705, 219, 12, activation=module)
    with pytest.raises(NotImplementedError):
        _cfg(module)


@pytest.mark.parametrize("module,spec", SUPPORTED, ids=IDS)
def test_make_net_config_writes_kind_and_parameters(module, spec, monkeypatch):
    cfg = _cfg(module)
    assert activation_spec(module) == spec
    assert cfg.activation == spec[0]
    assert cfg.act_alpha == pytest.approx(spec[1], rel=1e-7) and cfg.act_scale == pytest.approx(spec[2], rel=1e-7)
    # no kind changes the parameter count, nor the workspace of a path: fp32 is one path for all; at bf16 the fused kernels implement
    # ELU(1) only, so any other activation has the workspace of the layer-by-layer path (what HGYM_NO_FUSED gives the ELU net)
    assert _sizes(_cfg(module, "f32")) == _sizes(_cfg(None, "f32"))
    bf16 = _sizes(cfg)
    if spec == (L.ACT_ELU, 1.0, 1.0):
        assert bf16 == _sizes(_cfg())
    else:
        monkeypatch.setenv("HGYM_NO_FUSED", "1")
        assert bf16 == _sizes(_cfg())


def test_zero_filled_tail_is_the_elu_net():
    default = _cfg()
    assert (default.activation, default.act_alpha, default.act_scale) == (L.ACT_ELU, 1.0, 1.0)
    for precision in ("bf16", "f32"):
        z = _cfg(precision=precision)
        z.activation, z.act_alpha, z.act_scale = 0, 0.0, 0.0
        assert _sizes(z) == _sizes(_cfg(nn.ELU(), precision=precision))
        assert _sizes(z)[0] == 926105
    assert C.sizeof(L.NetConfig) == L.lib.hgym_sizeof(b"HgymNetConfig")


@pytest.mark.parametrize("kind,alpha,scale,msg", [
    (5, 0.0, 0.0, "activation=5: not one of"),
    (-1, 0.0, 0.0, "activation=-1: not one of"),
    (L.ACT_ELU, -1.0, 0.0, "must be finite and >= 0"),
    (L.ACT_SELU, 0.0, -1.0, "must be finite and >= 0"),
    (L.ACT_LEAKY_RELU, -0.01, 0.0, "must be finite and >= 0"),
    (L.ACT_ELU, float("nan"), 0.0, "must be finite and >= 0"),
    (L.ACT_LEAKY_RELU, 0.1, 2.0, "act_scale=2 is used by ELU / SELU only"),
    (L.ACT_TANH, 0.5, 0.0, "act_alpha=0.5 is not used by Tanh / Sigmoid"),
    (L.ACT_SIGMOID, 0.0, 1.0, "act_scale=1 is used by ELU / SELU only"),
])
def test_library_rejects_bad_kind_and_parameters(kind, alpha, scale, msg):
    cfg = _cfg()
    cfg.activation, cfg.act_alpha, cfg.act_scale = kind, alpha, scale
    for fn in (L.lib.hgym_net_param_count, L.lib.hgym_net_workspace_bytes):
        assert fn(C.byref(cfg)) < 0
        assert msg in L.lib.hgym_last_error().decode()


def test_export_of_a_tanh_policy_reloads_with_tanh(tmp_path):
    from humanoid.algo.ppo.actor_critic import ActorCritic
    from humanoid.utils.helpers import export_policy_as_jit
    ac = ActorCritic(705, 219, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128], activation=nn.Tanh())
    export_policy_as_jit(ac, str(tmp_path))
    m = torch.jit.load(str(tmp_path / "policy_1.pt"))
    kinds = [c.original_name for c in m.children()]
    assert kinds == ["Linear", "Tanh"] * 3 + ["Linear"]
    x = torch.randn(3, 705)
    with torch.no_grad():
        torch.testing.assert_close(m(x), ac.actor(x))
