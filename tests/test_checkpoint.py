"""humanoid.algo.ppo.checkpoint without a runner or a device: how the background path cuts a checkpoint out of a host snapshot
(assemble, param_layout), the atomic write, the sidecar's name, resolution and validation, and check_compatible's refusals."""
import os
import types

import pytest
import torch

from humanoid.algo.ppo import checkpoint as C
from hgym import _lib as L      # (slot names only: OPT_LR, OPT_STEP, NORM_HEADER_DOUBLES)

HYPER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False)       # PPO's _DeviceAdam.HYPER
SHAPES = [("std", (1,)), ("actor.0.weight", (7, 5)), ("actor.0.bias", (7,)), ("actor.2.weight", (3, 7)), ("actor.2.bias", (3,))]
P, K = 200, (5, 4)


def _snapshot(norm):
    """A host snapshot with distinct values everywhere, the state_dict of views into its parameter vector, and the dict it must become."""
    buf = dict(params=torch.arange(P, dtype=torch.float32) + 0.5, m=torch.arange(P, dtype=torch.float32) * -2.0,
               v=torch.arange(P, dtype=torch.float32) * 3.0 + 1000.0, opt=torch.arange(16, dtype=torch.float64) * 0.125 + 7.0)
    views, off = {}, 3      # (the entries do not start at 0 and leave gaps: the cut is by offset)
    for name, shape in SHAPES:
        n = int(torch.Size(shape).numel())
        views[name] = buf["params"][off:off + n].view(shape)
        off += n + 2
    want_state = {}
    for i, (name, shape) in enumerate(SHAPES):
        o = views[name].storage_offset()
        n = views[name].numel()
        want_state[i] = dict(step=torch.tensor(float(buf["opt"][L.OPT_STEP])), exp_avg=(torch.arange(o, o + n, dtype=torch.float32) * -2.0).view(shape),
                             exp_avg_sq=(torch.arange(o, o + n, dtype=torch.float32) * 3.0 + 1000.0).view(shape))
    want = {"model_state_dict": {k: v.clone() for k, v in views.items()},
            "optimizer_state_dict": dict(state=want_state, param_groups=[dict(lr=float(buf["opt"][L.OPT_LR]), **HYPER, params=[0, 1, 2, 3, 4])]),
            "iter": 11, "infos": {"note": "x"}}
    spec = None
    if norm:
        H = L.NORM_HEADER_DOUBLES
        buf["norm"] = torch.arange(H + 2 * sum(K), dtype=torch.float64) * 0.25 + 100.0
        nb, spec = buf["norm"], (K, (1e-2, 500))
        want["obs_norm_state_dict"] = dict(mean=nb[H:H + 5].clone(), var=nb[H + 5:H + 10].clone(), count=float(nb[2]), eps=1e-2, until=500)
        want["critic_obs_norm_state_dict"] = dict(mean=nb[H + 10:H + 14].clone(), var=nb[H + 14:H + 18].clone(), count=float(nb[3]), eps=1e-2, until=500)
    opt_layout = [(views[name].storage_offset(), shape) for name, shape in SHAPES]
    return buf, views, opt_layout, spec, want


def _assert_same(a, b, where="checkpoint"):
    """Same keys in the same order, tensors torch.equal (dtype and shape too), everything else ==."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _assert_same(a[k], b[k], "%s[%r]" % (where, k))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, "%s[%d]" % (where, i))
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


@pytest.mark.parametrize("norm", [False, True])
def test_assembled_checkpoint_equals_the_hand_built_one(tmp_path, norm):
    buf, views, opt_layout, spec, want = _snapshot(norm)
    layout = C.param_layout(views, buf["params"])
    assert layout == [(name, views[name].storage_offset(), shape) for name, shape in SHAPES]
    ck = C.assemble(buf, layout, opt_layout, HYPER, 11, {"note": "x"}, spec)
    assert list(ck) == ["model_state_dict", "optimizer_state_dict", "iter", "infos"] + (list(C.NORM_KEYS) if norm else [])
    _assert_same(want, ck)
    assert ck["optimizer_state_dict"]["param_groups"][0] == dict(lr=float(buf["opt"][L.OPT_LR]), **HYPER, params=[0, 1, 2, 3, 4])
    # views into the snapshot, not copies
    ptr = lambda t: t.untyped_storage().data_ptr()
    assert all(ptr(t) == ptr(buf["params"]) for t in ck["model_state_dict"].values())
    for st in ck["optimizer_state_dict"]["state"].values():
        assert ptr(st["exp_avg"]) == ptr(buf["m"]) and ptr(st["exp_avg_sq"]) == ptr(buf["v"])
    # through the file and back; the sidecar goes first and nothing temporary stays behind
    path = str(tmp_path / "model_11.pt")
    C.write_checkpoint(ck, path, dict(env={"x": torch.ones(2)}, iterations_done=12))
    _assert_same(want, torch.load(path, map_location="cpu"))
    assert sorted(os.listdir(str(tmp_path))) == ["envstate_11.pt", "model_11.pt"]
    C.write_atomic(ck, path)      # over an existing file
    _assert_same(want, torch.load(path, map_location="cpu"))
    assert sorted(os.listdir(str(tmp_path))) == ["envstate_11.pt", "model_11.pt"]


def test_layout_refuses_what_is_not_an_fp32_view_of_the_vector():
    big = torch.zeros(120)
    params = big[:100]
    C.param_layout({"a": params[90:100].view(2, 5)}, params)
    with pytest.raises(AssertionError, match="b lies outside"):
        C.param_layout({"a": params[:4], "b": big[90:110]}, params)
    with pytest.raises(AssertionError, match="a lies outside"):
        C.param_layout({"a": big[:10]}, big[4:])
    with pytest.raises(AssertionError, match="w is not an fp32 view"):
        C.param_layout({"w": torch.zeros(4, dtype=torch.float64)}, params)
    with pytest.raises(AssertionError, match="w is not an fp32 view"):
        C.param_layout({"w": params[:12].view(3, 4).t()}, params)


def test_sidecar_resolution(tmp_path, capsys):
    holder = types.SimpleNamespace(_warned_env_state=False)
    model = str(tmp_path / "model_3.pt")
    side = str(tmp_path / "envstate_3.pt")
    assert C.resolve_sidecar(model, None, 1, holder) is None                       # none beside the model file
    assert C.resolve_sidecar(model, str(tmp_path / "elsewhere.pt"), 1, holder) == str(tmp_path / "elsewhere.pt")     # (load() fails on it)
    open(side, "wb").close()
    assert C.resolve_sidecar(model, None, 1, holder) == side
    assert C.resolve_sidecar(model, False, 1, holder) is None
    assert C.resolve_sidecar(model, side, 1, holder) == side
    assert capsys.readouterr().out == "" and not holder._warned_env_state
    assert C.resolve_sidecar(model, None, 2, holder) is None and C.resolve_sidecar(model, side, 2, holder) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "envstate_3.pt is not loaded in a data-parallel run (world size 2)" in out
    # the save side shares the flag: said once per runner, whichever side says it
    assert C.exact_resume_on({"exact_resume": True}, 2, holder) is False and capsys.readouterr().out == ""
    fresh = types.SimpleNamespace(_warned_env_state=False)
    assert C.exact_resume_on({}, 2, fresh) is False and C.exact_resume_on({"exact_resume": False}, 1, fresh) is False
    assert capsys.readouterr().out == ""
    assert C.exact_resume_on({"exact_resume": True}, 1, fresh) is True
    assert C.exact_resume_on({"exact_resume": True}, 2, fresh) is False and C.exact_resume_on({"exact_resume": True}, 2, fresh) is False
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "env state is not saved in a data-parallel run (world size 2)" in out


def test_sidecar_validation():
    seen = []
    env = types.SimpleNamespace(check_state_dict=seen.append)
    side = dict(env={"meta": 1}, iterations_done=4, num_steps_per_env=60, world_size=1, rank=0)
    C.check_sidecar(side, 60, env)
    assert seen == [side["env"]]
    with pytest.raises(ValueError, match="env state: world_size is 2 in the sidecar; exact resume covers one rank"):
        C.check_sidecar(dict(side, world_size=2), 60, env)
    with pytest.raises(ValueError, match="env state: num_steps_per_env is 60 in the sidecar, 24 here"):
        C.check_sidecar(side, 24, env)
    assert seen == [side["env"]]      # (the env is asked last)


def _policy(noise="scalar", norm=False):
    return types.SimpleNamespace(noise_std_type=noise, empirical_normalization=norm, obs_norm_spec=(1e-2, None))


def test_check_compatible_refuses_by_name():
    ck = lambda first, **extra: dict({"model_state_dict": {first: torch.ones(3), "actor.0.weight": torch.ones(2, 2)}}, **extra)
    C.check_compatible(ck("std"), _policy("scalar"), None, "model_7.pt")
    C.check_compatible(ck("log_std"), _policy("log"), None, "model_7.pt")
    C.check_compatible(ck("std"), types.SimpleNamespace(), None, "model_7.pt")      # the reference's policy: scalar, no normaliser
    with pytest.raises(RuntimeError, match=r'model_7\.pt was trained with noise_std_type="log" \(its model_state_dict has `log_std`\).*built with noise_std_type="scalar"'):
        C.check_compatible(ck("log_std"), _policy("scalar"), None, "model_7.pt")
    with pytest.raises(RuntimeError, match=r'model_7\.pt was trained with noise_std_type="scalar" \(its model_state_dict has `std`\).*built with noise_std_type="log"'):
        C.check_compatible(ck("std"), _policy("log"), None, "model_7.pt")
    # the normaliser's keys (the cases themselves: tests/test_obs_norm.py), behind the noise check
    stats = {k: dict(mean=torch.zeros(2), var=torch.ones(2), count=3.0, eps=1e-2, until=None) for k in C.NORM_KEYS}
    C.check_compatible(ck("std", **stats), _policy(norm=True), None, "model_7.pt")
    with pytest.raises(RuntimeError, match=r"model_7\.pt carries `obs_norm_state_dict`"):
        C.check_compatible(ck("std", **stats), _policy(), None, "model_7.pt")
    with pytest.raises(RuntimeError, match="noise_std_type"):
        C.check_compatible(ck("log_std", **stats), _policy(), None, "model_7.pt")
    # RND, last
    with pytest.raises(RuntimeError, match=r"model_7\.pt carries rnd_state_dict"):
        C.check_compatible(ck("std", **{C.RND_STATE_KEY: {}}), _policy(), None, "model_7.pt")
    with pytest.raises(RuntimeError, match=r"model_7\.pt has no rnd_state_dict"):
        C.check_compatible(ck("std"), _policy(), types.SimpleNamespace(num_envs=8), "model_7.pt")
    with pytest.raises(RuntimeError, match="carries `obs_norm_state_dict`"):
        C.check_compatible(ck("std", **stats), _policy(), types.SimpleNamespace(num_envs=8), "model_7.pt")


def test_sidecar_name(tmp_path):
    """The cases of tests/test_env_state.py::test_sidecar_name_and_get_load_path, on the module's own function."""
    run = str(tmp_path / "Oct16_10-00-00_")
    for it in (0, 2):
        side = C.env_state_path(os.path.join(run, "model_%d.pt" % it))
        assert os.path.basename(side) == "envstate_%d.pt" % it and os.path.dirname(side) == run
    for name in ("sync.pt", "model_final.pt", "my_model.pt"):
        assert "model" not in os.path.basename(C.env_state_path(os.path.join(run, name))), name
