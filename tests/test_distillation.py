"""CPU: the host side of distillation -- the float64 reference of hgym_bc_grad against torch autograd, the
StudentTeacher policy's state dicts, every refusal of StudentTeacher / Distillation / hgym_bc_grad that needs no device, the task and the
script's teacher lookup."""
import ctypes as C
import inspect
import os

import pytest
import torch
import torch.nn as nn

import distill_common as D
from hgym import _lib as L


# ------------------------------------------------------------------------------------------------ the reference against autograd
def _autograd(seq, obs, target, loss_type, delta):
    seq.zero_grad()
    y = seq(obs)
    loss = nn.functional.mse_loss(y, target) if loss_type == "mse" else nn.functional.huber_loss(y, target, delta=delta)
    loss.backward()
    return float(loss), [p.grad.clone() for p in seq.parameters()]


def _plant(seq, obs, e):
    """Targets with mu - target close to e, and equal to it wherever a float64 target can give that: start from mu - e and take the
    rounding error of the difference out.  -> (target, the residuals as the loss will form them)."""
    with torch.no_grad():
        y = seq(obs)
        t = y - e
        for _ in range(4):
            t = t + ((y - t) - e)
        return t, y - t


@pytest.mark.parametrize("loss_type", D.LOSS_TYPES)
def test_reference_equals_float64_autograd(loss_type):
    from humanoid.algo.ppo.actor_critic import _mlp
    torch.manual_seed(3)
    delta, B, A = 0.75, 29, 12
    seq = _mlp([47, 40, 24, A], nn.ELU()).double()
    obs = torch.randn(B, 47, dtype=torch.float64)
    # residuals on both sides of delta, of both signs, and exactly at +-delta
    e = torch.randn(B, A, dtype=torch.float64) * 1.5 * delta
    e[0], e[1] = delta, -delta                  # twelve candidates each: the difference of two float64 numbers cannot hit every value
    e[2, 5], e[3, 7] = delta * (1 + 2.0 ** -40), delta * (1 - 2.0 ** -40)
    target, e = _plant(seq, obs, e)
    assert ((e.abs() < delta).any() and (e.abs() > delta).any() and (e == delta).any() and (e == -delta).any())
    want_loss, want = _autograd(seq, obs, target, loss_type, delta)
    layers = [(m.weight.detach(), m.bias.detach()) for m in seq if isinstance(m, nn.Linear)]
    loss, grads = D.bc_loss_and_grads(layers, obs, target, loss_type, delta)
    assert abs(float(loss) - want_loss) <= 1e-14 * max(1.0, abs(want_loss))
    for g, w in zip(D.flat(grads), want):
        assert D.rel_max(g, w) < 1e-12


def test_restated_update_walks_the_slices_in_storage_order():
    """distill_update: T / gradient_length slices per epoch, in order, one Adam step each; the first step of Adam moves every weight by
    lr * g / (|g| + eps): the bias corrections cancel."""
    layers = [(W.double(), b.double()) for W, b in D.make_layers("ragged")[0]]
    g = torch.Generator().manual_seed(1)
    N, T, G = 5, 4, 2
    obs = torch.randn(T * N, 47, generator=g).double()
    target = torch.randn(T * N, 12, generator=g).double()
    new, losses, opt = D.distill_update(layers, obs, target, N, G, 3, 1e-3)
    assert len(losses) == 3 * (T // G) and opt.t == 6
    one, l1, _ = D.distill_update(layers, obs[:G * N], target[:G * N], N, G, 1, 1e-3)
    want_loss, grads = D.bc_loss_and_grads(layers, obs[:G * N], target[:G * N])
    assert l1 == [float(want_loss)] and losses[0] == l1[0]
    for (W1, _), (W0, _), (gW, _) in zip(one, layers, grads):
        torch.testing.assert_close(W1 - W0, -1e-3 * gW / (gW.abs() + 1e-8), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ StudentTeacher
def _policy(**kw):
    from humanoid.algo import StudentTeacher
    return StudentTeacher(47, 19, 12, student_hidden_dims=[24, 16], teacher_hidden_dims=[40, 24, 16], critic_hidden_dims=[24, 8], **kw)


def _linear_keys(name, n):
    return ["%s.%d.%s" % (name, 2 * l, k) for l in range(n) for k in ("weight", "bias")]


def test_student_teacher_is_an_actor_critic_with_a_teacher_behind_it():
    from humanoid.algo import ActorCritic, StudentTeacher
    st = _policy()
    assert isinstance(st, ActorCritic) and not st.loaded_teacher
    assert list(st.state_dict()) == ["std"] + _linear_keys("actor", 3) + _linear_keys("critic", 3) + _linear_keys("teacher", 4)
    assert [m.out_features for m in st.actor if isinstance(m, nn.Linear)] == [24, 16, 12]
    assert [m.out_features for m in st.teacher if isinstance(m, nn.Linear)] == [40, 24, 16, 12]
    assert not any(p.requires_grad for p in st.teacher.parameters())
    assert float(st.std[0]) == pytest.approx(0.1)
    assert list(_policy(noise_std_type="log").state_dict())[0] == "log_std"
    sig = inspect.signature(StudentTeacher.__init__).parameters
    assert sig["student_hidden_dims"].default == [256, 128, 128] and sig["teacher_hidden_dims"].default == [512, 256, 128]
    assert sig["critic_hidden_dims"].default == [768, 256, 128] and sig["init_noise_std"].default == 0.1


def test_teacher_checkpoint_goes_into_the_teacher_and_nowhere_else():
    from humanoid.algo import ActorCritic
    torch.manual_seed(1)
    teacher = ActorCritic(47, 19, 12, actor_hidden_dims=[40, 24, 16], critic_hidden_dims=[32, 32], init_noise_std=0.7)
    st = _policy()
    before = {k: v.clone() for k, v in st.student_state_dict().items()}
    assert st.load_state_dict(teacher.state_dict()) is False and st.loaded_teacher
    for k, v in teacher.actor.state_dict().items():
        assert torch.equal(st.teacher.state_dict()[k].view(torch.int32), v.view(torch.int32)), k
    after = st.student_state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)      # std, student, critic untouched


def test_distillation_checkpoint_resumes_strictly():
    torch.manual_seed(2)
    a, b = _policy(), _policy()
    assert b.load_state_dict(a.state_dict()) is True and b.loaded_teacher
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    sd = a.state_dict()
    del sd["critic.0.bias"]
    with pytest.raises(RuntimeError, match="critic.0.bias"):
        _policy().load_state_dict(sd)


def test_teacher_shape_mismatch_is_refused_by_name():
    from humanoid.algo import ActorCritic
    wide = ActorCritic(47, 19, 12, actor_hidden_dims=[48, 24, 16], critic_hidden_dims=[8])
    st = _policy()
    with pytest.raises(RuntimeError, match=r"actor\.0\.weight has shape \(48, 47\), teacher\.0\.weight needs \(40, 47\)"):
        st.load_state_dict(wide.state_dict())
    shallow = ActorCritic(47, 19, 12, actor_hidden_dims=[40, 24], critic_hidden_dims=[8])
    with pytest.raises(RuntimeError, match=r"missing \['actor\.6\.bias', 'actor\.6\.weight'\]"):
        st.load_state_dict(shallow.state_dict())
    assert not st.loaded_teacher


def test_student_state_dict_is_a_ppo_checkpoint():
    from humanoid.algo import ActorCritic
    st = _policy()
    sd = st.student_state_dict()
    assert not any(k.startswith("teacher.") for k in sd) and len(sd) == len(st.state_dict()) - 8
    ac = ActorCritic(47, 19, 12, actor_hidden_dims=st.student_hidden_dims, critic_hidden_dims=[24, 8])
    ac.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in ac.state_dict().items())


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_student_teacher_refusals():
    with pytest.raises(ValueError, match="empirical_normalization"):
        _policy(empirical_normalization=True)
    with pytest.raises(ValueError, match="noise_std_type"):
        _policy(noise_std_type="softplus")
    with pytest.raises(RuntimeError, match="not bound"):
        _policy().teacher_inference(torch.zeros(1, 47))


def test_distillation_refusals():
    from humanoid.algo import Distillation, PPO, ActorCritic
    assert issubclass(Distillation, PPO)
    st = _policy()
    with pytest.raises(ValueError, match="loss_type"):
        Distillation(st, loss_type="l1")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="huber_delta"):
            Distillation(st, loss_type="huber", huber_delta=bad)
    with pytest.raises(ValueError, match="gradient_length"):
        Distillation(st, gradient_length=0)
    with pytest.raises(RuntimeError, match="no CPU training path"):      # PPO's own: the hot path is the device's
        Distillation(st, device="cpu")
    check = Distillation.check_setup
    check(st, 60, 15)
    with pytest.raises(ValueError, match="one rank"):
        check(st, 60, 15, world=2)
    with pytest.raises(ValueError, match="symmetry"):
        check(st, 60, 15, symmetry=object())
    with pytest.raises(ValueError, match="mirror_loss_coef"):
        check(st, 60, 15, mirror_loss_coef=0.5)
    for mode in ("minibatch", "none"):
        with pytest.raises(ValueError, match="advantage_normalization"):
            check(st, 60, 15, advantage_normalization=mode)
    with pytest.raises(ValueError, match="StudentTeacher"):
        check(ActorCritic(47, 19, 12, actor_hidden_dims=[8], critic_hidden_dims=[8]), 60, 15)
    with pytest.raises(ValueError, match="not a multiple of gradient_length=16"):
        check(st, 60, 16)
    alg = Distillation.__new__(Distillation)
    for call in (alg.diagnostics, alg.diagnostics_prepare):
        with pytest.raises(RuntimeError, match="no PPO diagnostics"):
            call()
    assert alg.update_capturable() is False
    sig = inspect.signature(Distillation.__init__).parameters
    assert list(sig)[1:] == ["policy", "num_learning_epochs", "gradient_length", "learning_rate", "max_grad_norm", "loss_type",
                             "huber_delta", "device"]
    assert (sig["gradient_length"].default, sig["max_grad_norm"].default, sig["loss_type"].default) == (15, None, "mse")


# ------------------------------------------------------------------------------------------------ the library's refusals
def _bc_call(loss_type=L.BC_MSE, delta=1.0, B=8, target=True, sums=True, max_batch=64):
    """hgym_bc_grad with fake (never dereferenced) addresses: every refusal comes before anything is launched or read."""
    from hgym import make_net_config
    cfg = make_net_config(47, 19, 12, [40, 24], [24], "f32", max_batch)
    fake = lambda ty: C.cast(C.c_void_p(0x1000), ty)
    batch = L.Batch()
    batch.obs, batch.idx, batch.B, batch.num_rows = fake(L.c_float_p), fake(L.c_i64_p), B, 100
    rc = L.lib.hgym_bc_grad(C.byref(cfg), C.byref(L.BCConfig(loss_type, delta)), C.byref(L.Net()), C.byref(batch),
                            fake(L.c_float_p) if target else None, fake(L.c_f64_p) if sums else None, None)
    return rc, L.lib.hgym_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(target=False), "null target"), (dict(sums=False), "null target / sums"),
    (dict(loss_type=2), "loss_type=2"), (dict(loss_type=-1), "loss_type=-1"),
    (dict(loss_type=L.BC_HUBER, delta=0.0), "huber_delta=0"), (dict(loss_type=L.BC_HUBER, delta=-1.0), "huber_delta=-1"),
    (dict(loss_type=L.BC_HUBER, delta=float("inf")), "huber_delta=inf"), (dict(loss_type=L.BC_HUBER, delta=float("nan")), "huber_delta="),
    (dict(B=0), "B=0"), (dict(B=-3), "B=-3"), (dict(B=65), "B=65 outside [1, max_batch = 64]"),
])
def test_bc_grad_refuses_before_anything_is_launched(kw, word):
    rc, msg = _bc_call(**kw)
    assert rc == -1 and word in msg, (rc, msg)      # HGYM_E_BADARG


def test_bc_grad_passes_its_own_checks_with_good_arguments():
    """The same call with nothing wrong reaches the net's own checks (a zero-filled HgymNet: null params), i.e. none of the above fired."""
    for kw in (dict(), dict(loss_type=L.BC_HUBER, delta=0.5), dict(B=64), dict(B=1)):
        rc, msg = _bc_call(**kw)
        assert rc == -1 and "null params / workspace" in msg, (rc, msg)
    assert L.lib.hgym_bc_grad(None, None, None, None, None, None, None) == -1


def test_bc_config_struct_and_python_mirror():
    from hgym import make_bc_config
    assert L.lib.hgym_sizeof(b"HgymBCConfig") == C.sizeof(L.BCConfig) == 8
    assert L.STRUCTS["HgymBCConfig"] is L.BCConfig and "hgym_bc_grad" in L.SYMBOLS
    c = make_bc_config("huber", 0.25)
    assert (c.loss_type, c.huber_delta) == (L.BC_HUBER, 0.25) and make_bc_config().loss_type == L.BC_MSE
    with pytest.raises(ValueError):
        make_bc_config("l1")
    with pytest.raises(ValueError):
        make_bc_config("huber", 0.0)


# ------------------------------------------------------------------------------------------------ task, config, script
def test_task_and_train_config():
    from humanoid.algo import Distillation, StudentTeacher
    from humanoid.algo.ppo.on_policy_runner import _split_algorithm_cfg, _split_policy_cfg
    from humanoid.envs import XBotLCfgPPO, XBotLDistillCfgPPO, XBotLFreeEnv, task_registry
    from humanoid.utils import class_to_dict
    assert task_registry.get_task_class("humanoid_distill") is XBotLFreeEnv
    cfg = class_to_dict(task_registry.get_cfgs("humanoid_distill")[1])
    assert cfg["runner"]["policy_class_name"] == "StudentTeacher" and cfg["runner"]["algorithm_class_name"] == "Distillation"
    assert cfg["runner"]["experiment_name"] == "XBot_e2e_distill" and cfg["teacher_experiment_name"] == XBotLCfgPPO.runner.experiment_name
    assert cfg["policy"]["teacher_hidden_dims"] == XBotLCfgPPO.policy.actor_hidden_dims and cfg["policy"]["student_hidden_dims"] == [256, 128, 128]
    kwargs, symmetry = _split_algorithm_cfg(cfg["algorithm"])
    assert kwargs == cfg["algorithm"] and not symmetry      # nothing taken out, nothing added
    params = inspect.signature(Distillation.__init__).parameters
    assert set(kwargs) <= set(params) - {"self", "policy", "device"}
    assert cfg["runner"]["num_steps_per_env"] % kwargs["gradient_length"] == 0
    assert set(_split_policy_cfg(cfg["policy"], cfg["runner"])) <= set(inspect.signature(StudentTeacher.__init__).parameters)
    assert isinstance(XBotLDistillCfgPPO(), XBotLCfgPPO)
    import sys
    R = sys.modules["humanoid.algo.ppo.on_policy_runner"]
    assert R.StudentTeacher is StudentTeacher and R.Distillation is Distillation      # visible to the runner's eval


def test_distill_script_finds_the_teacher_in_the_ppo_experiment(tmp_path):
    import importlib.util
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("distill_script", os.path.join(here, "humanoid-gym_amd", "humanoid", "scripts", "distill.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for run, its in (("Oct01_10-00-00_", (0, 100)), ("Oct02_09-00-00_", (0, 50, 200))):
        os.makedirs(tmp_path / run)
        for it in its:
            (tmp_path / run / ("model_%d.pt" % it)).write_bytes(b"")
    cfg = task_registry.get_cfgs("humanoid_distill")[1]
    path = lambda *argv: os.path.relpath(mod.teacher_path(cfg, get_args(["--task=humanoid_distill"] + list(argv)), str(tmp_path)), tmp_path)
    assert path() == os.path.join("Oct02_09-00-00_", "model_200.pt")
    assert path("--checkpoint", "50") == os.path.join("Oct02_09-00-00_", "model_50.pt")
    assert path("--load_run", "Oct01_10-00-00_") == os.path.join("Oct01_10-00-00_", "model_100.pt")
    with pytest.raises(ValueError, match="No runs"):
        mod.teacher_path(cfg, get_args(["--task=humanoid_distill"]), str(tmp_path / "nowhere"))
