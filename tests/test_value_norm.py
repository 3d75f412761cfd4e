"""CPU-only: value-target normalisation (PPO.value_normalization) as far as it needs no device.

1. The restatement (tests/value_norm_common.py): rsl_rl's merge over k batches IS the pooled update -- the population statistics of the
   concatenation -- in float64 to 1e-12, from the initial state and from a state that already holds data; the two fp32 maps undo each other
   to rounding.
2. The library's argument checks through ctypes: every refusal returns its code with nothing launched (there is no device here).
3. PPO.check_setup's new refusals, the calls tests/test_log_block.py makes, Distillation's refusal; the log block's new part on the same
   kind of stand-ins; the train config's keys; check_compatible's three refusals by key name; the host's ValueNormalizer."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import value_norm_common as V
from hgym import _lib as L
from humanoid.algo import PPO, Distillation
from humanoid.algo.ppo import checkpoint as ckpt
from humanoid.algo.ppo.log_block import LogBlock
from humanoid.algo.ppo.normalizer import ValueNormalizer
from humanoid.algo.ppo.smoothness import Smoothness


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("sizes", [(1,), (7, 1, 1000), (512, 512, 512), (3, 4096, 17, 1)], ids=str)
@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (10.0, 1.0), (-3.0, 0.25), (100.0, 0.01)], ids=str)
def test_merge_over_batches_is_the_pooled_update(sizes, mean, std):
    rng = np.random.default_rng(len(sizes) * 1000 + int(mean))
    batches = [(mean + std * rng.standard_normal(n) + 0.1 * std * k).astype(np.float32) for k, n in enumerate(sizes)]
    state = V.INITIAL
    for b in batches:
        state = V.merge(state, V.batch_stats(b))
    n, m, v = V.batch_stats(np.concatenate(batches))
    assert state[0] == n == float(sum(sizes))
    assert V.rel(state[1], m) <= 1e-12, (state, m)
    assert abs(state[2] - v) <= 1e-12 * max(v, 1e-300) if v > 0 else state[2] == 0.0, (state, v)
    # from the initial state one merge gives the batch's statistics themselves, bit for bit
    assert V.merge(V.INITIAL, V.batch_stats(batches[0]))[1:] == V.batch_stats(batches[0])[1:]


def test_merge_into_a_state_that_holds_data_and_a_constant_batch():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(300).astype(np.float32), np.full(200, 2.5, dtype=np.float32)
    assert V.batch_stats(b) == (200.0, 2.5, 0.0)
    state = V.merge(V.merge(V.INITIAL, V.batch_stats(a)), V.batch_stats(b))
    n, m, v = V.batch_stats(np.concatenate((a, b)))
    assert state[0] == n and V.rel(state[1], m) <= 1e-12 and V.rel(state[2], v) <= 1e-12
    only = V.merge(V.INITIAL, V.batch_stats(b))
    assert only == (200.0, 2.5, 0.0)
    y = V.normalize(b, only)
    assert y.dtype == np.float32 and np.all(y == 0.0) and np.all(np.isfinite(V.denormalize(y, only)))      # scale_f = eps: finite


def test_the_two_maps_undo_each_other_to_rounding():
    rng = np.random.default_rng(6)
    x = (5.0 + 2.0 * rng.standard_normal(1000)).astype(np.float32)
    state = V.merge(V.INITIAL, V.batch_stats(x))
    mean_f, scale_f = V.floats(state)
    assert mean_f.dtype == scale_f.dtype == np.float32 and float(scale_f) == float(np.float32(np.float32(np.sqrt(state[2])) + np.float32(1e-2)))
    back = V.denormalize(V.normalize(x, state), state)
    assert back.dtype == np.float32 and np.max(np.abs(back - x)) <= 4 * 2.0 ** -24 * np.max(np.abs(x))


def test_scratch_macro_mirrors_agree():
    for n in (1, 1023, 1024, 1025, 2049, 245760, 1024 * 1024 + 1):
        assert L.value_norm_scratch_doubles(n) == V.scratch_doubles(n)
    assert (L.VALUE_NORM_CHUNK, L.VALUE_NORM_MAX_BLOCKS, L.VALUE_NORM_BLOCK_DOUBLES) == (V.CHUNK, V.MAX_BLOCKS, 3)
    hdr = open(__file__.replace("tests/test_value_norm.py", "include/hgym.h")).read()
    for name, value in (("BLOCK_DOUBLES", 3), ("CHUNK", V.CHUNK), ("MAX_BLOCKS", V.MAX_BLOCKS), ("BATCH", L.VALUE_NORM_BATCH),
                        ("TICKET", L.VALUE_NORM_TICKET), ("PARTIALS", L.VALUE_NORM_PARTIALS)):
        assert re.search(r"#define HGYM_VALUE_NORM_%s %d\b" % (name, value), hdr), name


# ------------------------------------------------------------------------------------------------ 2. the library's argument checks
def _p(addr, kind=L.c_float_p):
    return C.cast(C.c_void_p(addr), kind)


F, D = 0x10000, 0x20000      # never dereferenced: every call below is refused before anything is launched
BAD, SHAPE = -1, -2          # HGYM_E_BADARG, HGYM_E_SHAPE


def test_library_refuses_bad_arguments_with_nothing_launched():
    lib = L.lib
    f, d, s = _p(F), _p(D, L.c_f64_p), _p(D + 0x1000, L.c_f64_p)
    nul_f, nul_d = None, None
    cases = [
        ("n = 0", SHAPE, lambda: lib.hgym_value_denormalize(0, f, f, d, 1e-2, None)),
        ("n < 0", SHAPE, lambda: lib.hgym_value_normalize(-5, f, d, 1e-2, None)),
        ("n = 0 (merge)", SHAPE, lambda: lib.hgym_value_norm_merge(0, f, d, s, None)),
        ("null src", BAD, lambda: lib.hgym_value_denormalize(8, nul_f, f, d, 1e-2, None)),
        ("null dst", BAD, lambda: lib.hgym_value_denormalize(8, f, nul_f, d, 1e-2, None)),
        ("null block", BAD, lambda: lib.hgym_value_denormalize(8, f, f, nul_d, 1e-2, None)),
        ("null x", BAD, lambda: lib.hgym_value_normalize(8, nul_f, d, 1e-2, None)),
        ("null block (normalize)", BAD, lambda: lib.hgym_value_normalize(8, f, nul_d, 1e-2, None)),
        ("null returns", BAD, lambda: lib.hgym_value_norm_merge(8, nul_f, d, s, None)),
        ("null block (merge)", BAD, lambda: lib.hgym_value_norm_merge(8, f, nul_d, s, None)),
        ("null scratch", BAD, lambda: lib.hgym_value_norm_merge(8, f, d, nul_d, None)),
        ("eps < 0", BAD, lambda: lib.hgym_value_denormalize(8, f, f, d, -1e-2, None)),
        ("eps = inf", BAD, lambda: lib.hgym_value_denormalize(8, f, f, d, float("inf"), None)),
        ("eps = nan", BAD, lambda: lib.hgym_value_normalize(8, f, d, float("nan"), None)),
        ("eps < 0 (normalize)", BAD, lambda: lib.hgym_value_normalize(8, f, d, -1.0, None)),
        ("misaligned block", BAD, lambda: lib.hgym_value_denormalize(8, f, f, _p(D + 4, L.c_f64_p), 1e-2, None)),
        ("misaligned block (normalize)", BAD, lambda: lib.hgym_value_normalize(8, f, _p(D + 4, L.c_f64_p), 1e-2, None)),
        ("misaligned block (merge)", BAD, lambda: lib.hgym_value_norm_merge(8, f, _p(D + 4, L.c_f64_p), s, None)),
        ("misaligned scratch", BAD, lambda: lib.hgym_value_norm_merge(8, f, d, _p(D + 0x1004, L.c_f64_p), None)),
        ("partial overlap", BAD, lambda: lib.hgym_value_denormalize(8, f, _p(F + 16), d, 1e-2, None)),
    ]
    for what, code, call in cases:
        assert call() == code, what
        assert L.lib.hgym_last_error(), what


# ------------------------------------------------------------------------------------------------ 3. PPO, the log block, configs, checkpoints
OK = dict(num_envs=64, num_transitions_per_env=8, num_mini_batches=2, num_actor_obs=5)


def test_check_setup_refusals_and_the_calls_of_the_log_block_tests():
    sym = object()
    # what tests/test_log_block.py calls, positionally and by keyword, with the new parameters left at their defaults
    PPO.check_setup(**OK)
    PPO.check_setup(64, 8, 2, 5)
    PPO.check_setup(64, 8, 2, 5, 1, None, True, 0.0, "batch", None, None)
    PPO.check_setup(**dict(OK, symmetry=sym, mirror_loss_coef=0.5, advantage_normalization="minibatch"))
    PPO.check_setup(**dict(OK, rnd=object(), smoothness=dict(temporal_coef=1.0), advantage_normalization="none"))
    # on: everything else combines
    PPO.check_setup(**dict(OK, value_normalization=True))
    PPO.check_setup(**dict(OK, value_normalization=True, value_normalization_eps=0.0, symmetry=sym, mirror_loss_coef=0.5, advantage_normalization="minibatch"))
    PPO.check_setup(**dict(OK, value_normalization=True, rnd=object(), smoothness=dict(temporal_coef=1.0), advantage_normalization="none"))
    PPO.check_setup(**dict(OK, value_normalization=False, world=2, value_normalization_eps=-1.0))      # off: nothing of it is looked at
    with pytest.raises(ValueError, match=re.escape("PPO.value_normalization runs on one rank (world size 2)")):
        PPO.check_setup(**dict(OK, value_normalization=True, world=2))
    for bad in (-1e-2, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=re.escape("PPO.value_normalization_eps=%r: must be finite and >= 0" % (bad,))):
            PPO.check_setup(**dict(OK, value_normalization=True, value_normalization_eps=bad))
    # the earlier refusals still win
    with pytest.raises(ValueError, match="one of batch, minibatch, none"):
        PPO.check_setup(**dict(OK, value_normalization=True, world=2, advantage_normalization="x"))
    assert PPO.value_normalization is False and PPO.value_normalization_eps == 1e-2


def test_distillation_refuses_value_normalization_before_any_device():
    a = Distillation.__new__(Distillation)
    a._world, a.gradient_length, a.actor_critic, a.value_normalization = 1, 4, SimpleNamespace(num_actor_obs=5), True
    with pytest.raises(ValueError, match=re.escape("PPO.value_normalization does not support Distillation")):
        a.init_storage(64, 8, [5], [5], [3])


def test_log_block_part_and_its_readers_on_stand_ins():
    opt = torch.arange(1.0, L.OPT_STATE + 1.0, dtype=torch.float64)
    smooth = torch.tensor([41.0, 42.0, 43.0, 44.0], dtype=torch.float64)
    block3 = torch.tensor([512.0, 1.5, 4.0], dtype=torch.float64)
    # stand-ins in tests/test_log_block.py's way: the options that are on, made without a device
    sm, vn = object.__new__(Smoothness), ValueNormalizer(block3, 1e-2)
    sm.sums = smooth
    old = SimpleNamespace(net=SimpleNamespace(opt_state=opt), _options=(sm,))
    assert [n for n, _ in PPO._log_parts(old)] == ["opt", "smooth"]
    on = SimpleNamespace(net=SimpleNamespace(opt_state=opt), _options=(sm, vn))
    assert [n for n, _ in PPO._log_parts(on)] == ["opt", "smooth", "value_norm"]      # behind smooth
    on._log = LogBlock(PPO._log_parts(on))
    block = on._log.device()
    assert block.numel() == L.OPT_STATE + 4 + 3 and torch.equal(block[-3:], block3)
    assert vn.last is None and vn.read_log(on._log.split(block)) == dict(count=512.0, mean=1.5, var=4.0, std=2.0) == vn.last
    old._log = LogBlock(PPO._log_parts(old))
    assert "value_norm" not in old._log.split(old._log.device())
    scal = SimpleNamespace(denoise_coef=0.0, last_denoise_loss=None, _scalar_order=())
    assert PPO.log_scalars(scal) == []      # (the option off)
    scal._scalar_order = (vn,)
    assert PPO.log_scalars(scal) == [("Policy/value_norm_mean", 1.5), ("Policy/value_norm_std", 2.0)]


def test_train_config_keys_are_not_constructor_arguments():
    from humanoid.algo.ppo.on_policy_runner import _split_algorithm_cfg, VALUE_NORM_KEYS
    assert VALUE_NORM_KEYS == ("value_normalization", "value_normalization_eps")
    kwargs, sym = _split_algorithm_cfg(dict(clip_param=0.2, value_normalization=True, value_normalization_eps=0.05))
    assert kwargs == dict(clip_param=0.2) and sym is False


def test_check_compatible_refuses_by_key_name():
    ac = SimpleNamespace(noise_std_type="scalar", empirical_normalization=False)
    plain = {"model_state_dict": {"std": torch.ones(3)}, "optimizer_state_dict": {}, "iter": 3, "infos": None}
    with_vn = dict(plain, **{ckpt.VALUE_NORM_KEY: dict(count=512.0, mean=0.5, var=2.0, eps=1e-2)})
    assert ckpt.VALUE_NORM_KEY == "value_norm_state_dict"
    ckpt.check_compatible(plain, ac, None, "model_3.pt")                       # the call as it was
    ckpt.check_compatible(plain, ac, None, "model_3.pt", value_norm=None)
    ckpt.check_compatible(with_vn, ac, None, "model_3.pt", value_norm=1e-2)
    with pytest.raises(RuntimeError, match=r"model_3.pt carries `value_norm_state_dict`: it was trained with PPO.value_normalization"):
        ckpt.check_compatible(with_vn, ac, None, "model_3.pt")
    with pytest.raises(RuntimeError, match=r"model_3.pt has no `value_norm_state_dict`: it was trained without PPO.value_normalization"):
        ckpt.check_compatible(plain, ac, None, "model_3.pt", value_norm=1e-2)
    with pytest.raises(RuntimeError, match=r"`value_norm_state_dict` was saved with value_normalization_eps=0.01; this run was built with 0.05"):
        ckpt.check_compatible(with_vn, ac, None, "model_3.pt", value_norm=0.05)
    # extra_entries: the key only with the option on
    off = SimpleNamespace(actor_critic=SimpleNamespace(), _rnd=None)
    assert ckpt.extra_entries(off) == {}
    on = SimpleNamespace(actor_critic=SimpleNamespace(), _rnd=None, value_normalizer=ValueNormalizer(torch.tensor([512.0, 0.5, 2.0], dtype=torch.float64), 1e-2))
    assert ckpt.extra_entries(on) == {ckpt.VALUE_NORM_KEY: dict(count=512.0, mean=0.5, var=2.0, eps=1e-2)}
    assert ckpt.value_norm_spec(off) is None and ckpt.value_norm_spec(on) == 1e-2


def test_host_value_normalizer():
    block = torch.tensor(V.INITIAL, dtype=torch.float64)
    vn = ValueNormalizer(block, 1e-2)
    assert (vn.count, float(vn.mean), float(vn.var), float(vn.std)) == (0, 0.0, 1.0, 1.0)
    vn.load_state_dict(dict(count=300.0, mean=5.0, var=4.0, eps=1e-2))
    assert torch.equal(block, torch.tensor([300.0, 5.0, 4.0], dtype=torch.float64)) and vn.state_dict() == dict(count=300.0, mean=5.0, var=4.0, eps=1e-2)
    assert vn.stats() == dict(count=300, mean=5.0, var=4.0, std=2.0) and vn.block is block      # one read for all four; the device tensor
    x = torch.tensor([1.0, 5.0, 9.0], dtype=torch.float64)
    y = vn.forward(x)
    assert torch.allclose(y, (x - 5.0) / 2.01, rtol=0, atol=1e-15) and torch.allclose(vn.inverse(y), x, rtol=0, atol=1e-14) and torch.equal(vn(x), y)
    x32 = x.float()
    want = torch.from_numpy(V.normalize(x32.numpy(), (300.0, 5.0, 4.0)))
    assert torch.equal(vn.forward(x32), want)      # in fp32 it is the device's map
    assert torch.equal(vn.inverse(want), torch.from_numpy(V.denormalize(want.numpy(), (300.0, 5.0, 4.0))))
