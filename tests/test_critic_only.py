"""CPU-only: critic-only training without a device -- the float64 restatement of the value loss against torch
autograd with ties planted on both operands of the max and on both clamp edges; the library's refusals on fabricated addresses; config
parsing and every refusal of PPO.critic_warmup_updates and Distillation.train_critic; the graph-key entry and its off value; the log
block's layout with the options on and off; the checkpoint key; the scripts' switches."""
import ctypes as C
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

import critic_only_common as CO
from hgym import _lib as L

f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the arithmetic
def _autograd(v, vold, ret, clip, unclipped):
    v = v.clone().requires_grad_(True)
    if unclipped:
        loss = (ret - v).pow(2)
    else:      # ppo.py:154-160 of the reference
        vc = vold + (v - vold).clamp(-clip, clip)
        loss = torch.max((v - ret).pow(2), (vc - ret).pow(2))
    loss.sum().backward()
    return loss.detach(), v.grad


def test_value_loss_restatement_equals_autograd_with_planted_ties():
    """clip = 1/4 and every number a multiple of 1/8: all differences are exact, so the ties are ties in float64.
      rows 0, 1   v - vold = +clip, -clip exactly: the clamp's closed edges (vc == v, a tie of the max: the gradient is that of (v - R)^2)
      rows 2, 3   v outside the clip range and R = (v + vc) / 2: (v - R)^2 == (vc - R)^2 with vc != v -- the max splits evenly and the
                  clamped half passes nothing: half the unclipped gradient -- on either side of the range
      row 4       v inside the range (vc == v): a tie again
      rows 5, 6   no tie: the clipped branch wins (gradient 0), the unclipped branch wins"""
    clip = 0.25
    vold = f64(1.0, 1.0, 0.0, 0.0, 0.5, 0.0, 0.0)
    v = f64(1.25, 0.75, 1.0, -1.0, 0.625, 1.0, 1.0)
    ret = f64(2.0, 2.0, 0.625, -0.625, 0.0, 2.0, 0.0)
    loss, grad = CO.vf_terms(v, vold, ret, clip, False)
    want_loss, want_grad = _autograd(v, vold, ret, clip, False)
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad), (grad, want_grad)
    vc = vold + (v - vold).clamp(-clip, clip)
    tie = (v - ret) ** 2 == (vc - ret) ** 2
    assert tie.tolist() == [True, True, True, True, True, False, False]
    assert torch.equal(grad[:2], 2 * (v - ret)[:2]) and torch.equal(grad[2:4], (v - ret)[2:4]) and float(grad[5]) == 0.0
    assert float(grad[6]) == float(2 * (v - ret)[6])
    loss, grad = CO.vf_terms(v, vold, ret, clip, True)
    want_loss, want_grad = _autograd(v, vold, ret, clip, True)
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)


@pytest.mark.parametrize("unclipped", [False, True])
def test_value_loss_restatement_on_random_values(unclipped):
    g = torch.Generator().manual_seed(4)
    v, vold, ret = (torch.randn(500, generator=g, dtype=torch.float64) for _ in range(3))
    loss, grad = CO.vf_terms(v, vold, ret, 0.2, unclipped)
    want_loss, want_grad = _autograd(v, vold, ret, 0.2, unclipped)
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)


@pytest.mark.parametrize("name", ["ragged", "ragged_tanh"])
@pytest.mark.parametrize("unclipped", [False, True])
def test_reference_gradient_is_autograd_through_the_critic(name, unclipped):
    """vf_loss_and_grads (the hand-written backward of oracle/ppo_oracle.py) against torch autograd through the same float64 MLP."""
    case, p = CO.make_case(name, 65), CO.make_params(name)
    idx = case["idx"]
    priv, vold, ret = case["cols"][1][idx].double(), case["cols"][3][idx].double(), case["cols"][5][idx].double()
    layers = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in p.critic]
    act = torch.tanh if CO.NETS[name][3] == "tanh" else torch.nn.functional.elu
    x = priv
    for l, (W, b) in enumerate(layers):
        x = x @ W.t() + b
        if l < len(layers) - 1:
            x = act(x)
    v = x.squeeze(-1)
    if unclipped:
        loss = ((v - ret) ** 2).mean()
    else:
        vc = vold + (v - vold).clamp(-CO.CLIP, CO.CLIP)
        loss = torch.max((v - ret) ** 2, (vc - ret) ** 2).mean()
    (CO.VALUE_COEF * loss).backward()
    got_loss, got = CO.vf_loss_and_grads([(W.detach(), b.detach()) for W, b in layers], priv, vold, ret, unclipped=unclipped, mlp=CO.mlp_fns(name))
    assert abs(float(got_loss) - float(loss.detach())) <= 1e-14 * float(loss.detach())
    for (dW, db), (W, b) in zip(got, layers):
        assert CO.rel_l2(dW, W.grad) <= 1e-13 and CO.rel_l2(db, b.grad) <= 1e-13


# ------------------------------------------------------------------------------------------------ the library, without a device
def test_struct_symbols_and_python_mirror():
    from hgym import make_vf_config
    assert L.lib.hgym_sizeof(b"HgymVFConfig") == C.sizeof(L.VFConfig) == 16 and L.STRUCTS["HgymVFConfig"] is L.VFConfig
    assert [n for n, _ in L.VFConfig._fields_] == ["clip_param", "value_coef", "unclipped", "keep_others"]
    for name in ("hgym_vf_grad", "hgym_bc_vf_grad"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    c = make_vf_config(0.25, 0.5, clipped_value_loss=True, keep_others=True)
    assert (c.clip_param, c.value_coef, c.unclipped, c.keep_others) == (0.25, 0.5, 0, 1)
    c = make_vf_config(float("nan"), 2.0, clipped_value_loss=False)      # the unclipped form does not read the clip range
    assert (c.clip_param, c.unclipped, c.keep_others) == (0.0, 1, 0)
    for kw in (dict(clip_param=-0.1), dict(clip_param=float("nan")), dict(clip_param=float("inf")), dict(value_coef=-1.0),
               dict(value_coef=float("nan")), dict(value_coef=float("inf"))):
        with pytest.raises(ValueError):
            make_vf_config(**kw)
    with open(os.path.join(ROOT, "include", "hgym.h")) as f:
        header = f.read()
    assert "#define HGYM_VERSION 9 " in header and header.index("} HgymVFConfig;") > header.index("int32_t hgym_ppo_apply(")


def _fake(ty, a=0x1000):
    return C.cast(C.c_void_p(a), ty)


def _vf_call(combined=False, vf="good", B=8, max_batch=64, sums=0x3000, bc_sums=0x4000, target=0x5000, **members):
    """hgym_vf_grad / hgym_bc_vf_grad with fabricated (never dereferenced) addresses: every refusal comes before anything is launched."""
    from hgym import make_net_config
    cfg = make_net_config(47, 19, 12, [40, 24], [24], "f32", max_batch)
    batch = L.Batch()
    batch.obs, batch.priv, batch.values, batch.returns = (_fake(L.c_float_p, a) for a in (0x10000, 0x20000, 0x30000, 0x40000))
    batch.idx, batch.B, batch.num_rows = _fake(L.c_i64_p, 0x50000), B, 100
    for k, v in members.items():
        setattr(batch, k, v)
    v = L.VFConfig(0.2, 1.0, 0, 0) if vf == "good" else vf
    vp, sp = (None if v is None else C.byref(v)), (None if not sums else _fake(L.c_f64_p, sums))
    if combined:
        rc = L.lib.hgym_bc_vf_grad(C.byref(cfg), C.byref(L.BCConfig(L.BC_MSE, 1.0)), vp, C.byref(L.Net()), C.byref(batch),
                                   None if not target else _fake(L.c_float_p, target), None if not bc_sums else _fake(L.c_f64_p, bc_sums), sp, None)
    else:
        rc = L.lib.hgym_vf_grad(C.byref(cfg), vp, C.byref(L.Net()), C.byref(batch), sp, None)
    return rc, L.lib.hgym_last_error().decode()


nan, inf = float("nan"), float("inf")
REFUSALS = [
    (dict(sums=0), "sums must be non-null"), (dict(sums=0x3004), "8-byte aligned"), (dict(vf=None), "null cfg / "),
    (dict(vf=L.VFConfig(nan, 1.0, 0, 0)), "clip_param=nan"), (dict(vf=L.VFConfig(-0.5, 1.0, 0, 0)), "clip_param=-0.5"),
    (dict(vf=L.VFConfig(inf, 1.0, 0, 0)), "clip_param=inf"), (dict(vf=L.VFConfig(0.2, nan, 0, 0)), "value_coef=nan"),
    (dict(vf=L.VFConfig(0.2, -1.0, 0, 0)), "value_coef=-1"), (dict(vf=L.VFConfig(0.2, inf, 1, 0)), "value_coef=inf"),
    (dict(vf=L.VFConfig(0.2, 1.0, 2, 0)), "unclipped=2"), (dict(vf=L.VFConfig(0.2, 1.0, 0, -1)), "keep_others=-1"),
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(B=65), "B=65 outside [1, max_batch = 64]"),
    (dict(values=None), "needs HgymBatch.values"), (dict(returns=None), "null HgymBatch.priv / returns / idx"),
    (dict(priv=None), "null HgymBatch.priv / returns / idx"), (dict(idx=None), "null HgymBatch.priv / returns / idx"),
    (dict(priv_bf16=C.c_void_p(0x60008)), "misaligned"),
]


@pytest.mark.parametrize("combined", [False, True], ids=["vf_grad", "bc_vf_grad"])
@pytest.mark.parametrize("kw, word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_library_refuses_before_anything_is_launched(kw, word, combined):
    rc, msg = _vf_call(combined, **kw)
    assert rc == -1 and word in msg, (rc, msg)      # HGYM_E_BADARG


def test_library_passes_its_own_checks_with_good_arguments():
    """The same calls with nothing wrong reach the net's own checks (a zero-filled HgymNet: null params): none of the above fired.  The
    unclipped form needs neither `values` nor a valid clip range."""
    for combined in (False, True):
        for kw in (dict(), dict(B=64), dict(B=1), dict(vf=L.VFConfig(nan, 1.0, 1, 1), values=None), dict(vf=L.VFConfig(0.0, 0.0, 0, 1))):
            rc, msg = _vf_call(combined, **kw)
            assert rc == -1 and "null params / workspace" in msg, (combined, kw, rc, msg)
    for kw, word in ((dict(target=0), "null target / bc_sums"), (dict(bc_sums=0), "null target / bc_sums"), (dict(bc_sums=0x3000), "two blocks"),
                     (dict(obs=None), "null HgymBatch.obs"), (dict(obs_bf16=C.c_void_p(0x70004)), "misaligned obs_bf16")):
        rc, msg = _vf_call(True, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.lib.hgym_vf_grad(None, None, None, None, None, None) == -1
    assert L.lib.hgym_bc_vf_grad(None, None, None, None, None, None, None, None, None) == -1


def test_make_vf_batch_names_what_the_call_reads_and_nothing_else():
    from hgym import make_vf_batch
    priv, values, returns, obs = torch.zeros(10, 19), torch.zeros(10), torch.zeros(10), torch.zeros(10, 47)
    idx = torch.arange(4)
    b = make_vf_batch(priv, values, returns, idx)
    assert (b.B, b.num_rows) == (4, 10) and not b.obs and not b.actions and not b.advantages and not b.logp and not b.mu and not b.sigma
    assert C.addressof(b.priv.contents) == priv.data_ptr() and C.addressof(b.returns.contents) == returns.data_ptr() and not b.priv_bf16
    assert not make_vf_batch(priv, None, returns, idx).values
    b = make_vf_batch(priv, values, returns, idx, obs=obs, priv_bf16=torch.zeros(10, 128, dtype=torch.bfloat16))
    assert C.addressof(b.obs.contents) == obs.data_ptr() and b.priv_bf16 and not b.obs_bf16


# ------------------------------------------------------------------------------------------------ PPO.critic_warmup_updates
def test_warmup_parsing_and_refusals():
    from humanoid.algo import PPO
    from humanoid.algo.ppo import critic_warmup as W
    assert PPO.critic_warmup_updates == 0 and "critic_warmup_updates" not in inspect.signature(PPO.__init__).parameters
    assert [W.parse_config(v) for v in (None, 0, 3, 2.0)] == [0, 0, 3, 2]
    for bad in (-1, 1.5, True, "x"):
        with pytest.raises(ValueError):
            W.parse_config(bad)
    W.check_setup(1)
    with pytest.raises(ValueError, match="one rank"):
        W.check_setup(2)
    # an optimiser state with non-zero actor moments while updates remain
    z, one = torch.zeros(3), torch.ones(3)
    W.check_moments(2, [("std", z, z), ("actor.0.weight", z, z), ("critic.0.weight", one, one)])
    W.check_moments(0, [("actor.0.weight", one, one)])
    for name, m, v in (("std", one, z), ("log_std", z, one), ("actor.4.bias", one, one)):
        with pytest.raises(ValueError, match="non-zero Adam moments for `%s`" % name):
            W.check_moments(1, [("critic.0.weight", one, one), (name, m, v)])


def test_warmup_counts_graph_key_and_log_block():
    from hgym import make_ppo_config
    from humanoid.algo.ppo import critic_warmup as W
    from humanoid.algo.ppo.log_block import LogBlock
    ppo = make_ppo_config(clip_param=0.3, value_loss_coef=0.5, adaptive=True, grad_norm_ready=True, mirror_coef=0.25, clipped_value_loss=False)
    w = W.CriticWarmup(2, ppo, 0.3, 0.5, False, "cpu")
    assert (w.vf_cfg.value_coef, w.vf_cfg.unclipped, w.vf_cfg.keep_others) == (0.5, 1, 0)
    a = w.apply_cfg      # the run's own step, the learning-rate rule off, the norm from hgym_ppo_apply's own pass
    assert (a.adaptive_lr, a.grad_norm_ready) == (0, 0) and (ppo.adaptive_lr, ppo.grad_norm_ready) == (1, 1)
    assert (a.max_grad_norm, a.beta1, a.lr_max, a.world_size) == (ppo.max_grad_norm, ppo.beta1, ppo.lr_max, ppo.world_size)
    keys = []
    for _ in range(3):
        keys.append((w.remaining, w.active, w.graph_key()))
        if w.active:
            w.update_done()
    assert keys == [(2, True, dict(critic_warmup=True)), (1, True, dict(critic_warmup=True)), (0, False, dict(critic_warmup=False))]
    assert w.state_dict() == dict(done=2, updates=2)
    # the log part: sum of the value losses, their number, the updates remaining behind the last critic-only one
    opt = torch.arange(1.0, L.OPT_STATE + 1.0, dtype=torch.float64)
    log = LogBlock([("opt", opt)] + w.log_parts())
    assert log.numel() == L.OPT_STATE + 3 and list(log.split(log.device())) == ["opt", "critic_warmup"]
    w.block.copy_(f64(1.5, 4.0, 1.0))
    assert w.read_log(log.split(log.device())) == dict(value_loss=0.375, remaining=2, trained=True)
    assert w.log_scalars() == [("Policy/critic_warmup_remaining", 2.0)]
    w.block.zero_()      # retired: a plain update's log
    assert w.read_log(log.split(log.device())) == dict(value_loss=None, remaining=0, trained=False) and w.log_scalars() == []


def test_graph_key_has_the_entry_and_its_off_value():
    """PPO.update_graph_key lists every option's entry as it reads while the option is off; the option's own graph_key() fills it in."""
    from humanoid.algo import PPO
    src = inspect.getsource(PPO.update_graph_key)
    assert "critic_warmup=False" in src and src.index("critic_warmup=False") < src.index("guidance=None")      # (guidance stays last)
    assert PPO.__init__.__code__.co_names.count("_warmup") == 1      # off until init_storage reads the option


def test_checkpoint_key_and_its_refusals():
    from humanoid.algo.ppo import checkpoint as CK
    from humanoid.algo.ppo import critic_warmup as W
    assert CK.WARMUP_KEY == W.STATE_KEY == "critic_warmup_state_dict"
    sd = dict(done=1, updates=2)
    W.check_state_dict(sd, "model_1.pt", True)
    W.check_state_dict(None, "model_1.pt", False)
    with pytest.raises(RuntimeError, match="carries `critic_warmup_state_dict`"):
        W.check_state_dict(sd, "model_1.pt", False)
    with pytest.raises(RuntimeError, match="has no `critic_warmup_state_dict`"):
        W.check_state_dict(None, "model_1.pt", True)

    class Alg:      # extra_entries reads these and nothing else of a plain run
        class actor_critic:
            pass
        _rnd = value_normalizer = _guide = None

        class _warmup:
            state_dict = staticmethod(lambda: sd)
    assert CK.extra_entries(Alg) == {CK.WARMUP_KEY: sd}
    Alg._warmup = None
    assert CK.extra_entries(Alg) == {}
    loaded = dict(model_state_dict={"std": torch.ones(12)}, **{CK.WARMUP_KEY: sd})
    ac = SimpleNamespace(noise_std_type="scalar")
    CK.check_compatible(loaded, ac, None, "model_1.pt", critic_warmup=True)
    with pytest.raises(RuntimeError, match="carries `critic_warmup_state_dict`"):
        CK.check_compatible(loaded, ac, None, "model_1.pt")
    with pytest.raises(RuntimeError, match="has no `critic_warmup_state_dict`"):
        CK.check_compatible(dict(model_state_dict=loaded["model_state_dict"]), ac, None, "model_1.pt", critic_warmup=True)


# ------------------------------------------------------------------------------------------------ Distillation.train_critic
def test_train_critic_attribute_config_keys_and_log_layout():
    from humanoid.algo import Distillation
    from humanoid.algo.ppo import on_policy_runner as R
    from humanoid.algo.ppo.log_block import LogBlock
    assert Distillation.train_critic is False and "train_critic" not in inspect.signature(Distillation.__init__).parameters
    kw, sym = R._split_algorithm_cfg(dict(gradient_length=4, train_critic=True, critic_warmup_updates=3, value_loss_coef=0.5))
    assert kw == dict(gradient_length=4, value_loss_coef=0.5) and sym is False      # (value_loss_coef stays PPO's own argument)
    assert (R.TRAIN_CRITIC_KEY, R.WARMUP_KEY) == ("train_critic", "critic_warmup_updates")
    assert R.DISTILL_CRITIC_KEYS == ("value_loss_coef", "use_clipped_value_loss", "clip_param", "gamma", "lam")
    from humanoid.envs import XBotLCfgPPO, XBotLDistillCfgPPO
    assert not hasattr(XBotLDistillCfgPPO.algorithm, "train_critic") and not hasattr(XBotLCfgPPO.algorithm, "critic_warmup_updates")
    # the log block: opt | bc(2) with the option off, opt | bc(2) | vf(2) with it on
    opt, bc, vf = torch.arange(1.0, L.OPT_STATE + 1.0, dtype=torch.float64), f64(51.0, 2.0), f64(3.0, 4.0)
    off = SimpleNamespace(net=SimpleNamespace(opt_state=opt), _bc_sums=bc, _vf_sums=None)
    on = SimpleNamespace(net=SimpleNamespace(opt_state=opt), _bc_sums=bc, _vf_sums=vf)
    assert [n for n, _ in Distillation._log_parts(off)] == ["opt", "bc"] and [n for n, _ in Distillation._log_parts(on)] == ["opt", "bc", "vf"]
    log = LogBlock(Distillation._log_parts(on))
    block = log.device()
    assert torch.equal(block, torch.cat((opt, bc, vf))) and log.numel() == L.OPT_STATE + 4
    parts = log.split(block)
    assert torch.equal(parts["bc"], bc) and torch.equal(parts["vf"], vf)


def test_train_critic_refusals_stay():
    """What a cloning run refused it still refuses with the option on: value normalisation, several ranks, critic warm-up beside it."""
    from humanoid.algo import Distillation, StudentTeacher
    st = StudentTeacher(47, 19, 12, student_hidden_dims=[8], teacher_hidden_dims=[8], critic_hidden_dims=[8])
    with pytest.raises(ValueError, match="one rank"):
        Distillation.check_setup(st, 8, 4, world=2)
    src = inspect.getsource(Distillation.init_storage)
    assert "PPO.value_normalization does not support Distillation" in src and "PPO.critic_warmup_updates does not support Distillation" in src


def test_script_switches():
    for script, switch, key in (("train.py", "HGYM_CRITIC_WARMUP", "critic_warmup_updates"), ("distill.py", "HGYM_DISTILL_CRITIC", "train_critic")):
        with open(os.path.join(ROOT, "humanoid-gym_amd", "humanoid", "scripts", script)) as f:
            src = f.read()
        assert 'os.environ.get("%s"' % switch in src and "algorithm.%s = " % key in src, script
