"""CPU-only: PPO.advantage_normalization's host side -- the train config's keys, the mode check, and hgym_adv_normalize_minibatches'
argument validation, which answers before anything is launched (there is no GPU here).  tests/test_adv_norm_gpu.py has the kernel."""
import ctypes as C

import pytest

E_BADARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -4


def test_split_algorithm_cfg_takes_both_keys_out():
    from humanoid.algo.ppo.on_policy_runner import _split_algorithm_cfg
    cfg = dict(clip_param=0.2, symmetry=True, advantage_normalization="minibatch", normalize_advantage_per_mini_batch=True)
    before = dict(cfg)
    kwargs, symmetry = _split_algorithm_cfg(cfg)
    assert kwargs == dict(clip_param=0.2) and symmetry is True
    assert cfg == before      # the caller's dict is left alone
    assert _split_algorithm_cfg(dict(clip_param=0.2)) == (dict(clip_param=0.2), False)


@pytest.mark.parametrize("cfg,mode", [
    ({}, "batch"),
    ({"advantage_normalization": "batch"}, "batch"),
    ({"advantage_normalization": "minibatch"}, "minibatch"),
    ({"advantage_normalization": "none"}, "none"),
    ({"normalize_advantage_per_mini_batch": True}, "minibatch"),
    ({"normalize_advantage_per_mini_batch": False}, "batch"),
    ({"normalize_advantage_per_mini_batch": True, "advantage_normalization": "minibatch"}, "minibatch"),
    ({"normalize_advantage_per_mini_batch": False, "advantage_normalization": "batch"}, "batch"),
    ({"normalize_advantage_per_mini_batch": None, "advantage_normalization": "none"}, "none"),
])
def test_split_advantage_cfg(cfg, mode):
    from humanoid.algo.ppo.on_policy_runner import _split_advantage_cfg
    before = dict(cfg)
    assert _split_advantage_cfg(cfg) == mode
    assert cfg == before


@pytest.mark.parametrize("cfg", [
    {"normalize_advantage_per_mini_batch": True, "advantage_normalization": "batch"},
    {"normalize_advantage_per_mini_batch": True, "advantage_normalization": "none"},
    {"normalize_advantage_per_mini_batch": False, "advantage_normalization": "minibatch"},
    {"normalize_advantage_per_mini_batch": False, "advantage_normalization": "none"},
    {"advantage_normalization": "mini_batch"},
    {"advantage_normalization": True},
])
def test_split_advantage_cfg_refuses_disagreement_and_unknown_modes(cfg):
    from humanoid.algo.ppo.on_policy_runner import _split_advantage_cfg
    with pytest.raises(ValueError, match="advantage"):
        _split_advantage_cfg(cfg)


def test_ppo_declares_the_modes_and_defaults_to_batch():
    from humanoid.algo import PPO
    assert PPO.advantage_normalization == "batch"
    assert PPO.ADVANTAGE_NORMALIZATIONS == ("batch", "minibatch", "none")


def test_storage_compute_returns_takes_normalize():
    import inspect
    from humanoid.algo.ppo.rollout_storage import RolloutStorage
    p = inspect.signature(RolloutStorage.compute_returns).parameters
    assert p["normalize"].default is True


def test_library_exports_the_call_and_the_scratch_size():
    from hgym import _lib as L
    import hgym
    assert "hgym_adv_normalize_minibatches" in L.SYMBOLS and hasattr(L.lib, "hgym_adv_normalize_minibatches")
    assert callable(hgym.adv_normalize_minibatches)
    c = L.ADV_MB_CHUNK
    # per segment: sum, sum of squares, counter, and two doubles per chunk
    assert L.adv_mb_scratch_doubles(1, 2) == 5 and L.adv_mb_scratch_doubles(1, c) == 5 and L.adv_mb_scratch_doubles(1, c + 1) == 7
    assert L.adv_mb_scratch_doubles(4, 61440) == 4 * (3 + 2 * 60)


def _ptr(addr, kind):
    return C.cast(C.c_void_p(addr), kind)


def _call(segments, seg_len, idx, adv, out, rows, scratch):
    from hgym import _lib as L
    rc = L.lib.hgym_adv_normalize_minibatches(segments, seg_len, idx, adv, out, rows, scratch, None)
    return rc, L.lib.hgym_last_error()


def test_arguments_are_validated_before_anything_is_launched():
    """Every refused call returns before the first launch, so it answers without a device.  The pointers of the later cases are made-up
    addresses: validation compares them, nothing reads through them."""
    from hgym import _lib as L
    rc, msg = _call(4, 1, None, None, None, 0, None)
    assert rc == E_SHAPE and b"seg_len=1" in msg
    rc, msg = _call(0, 64, None, None, None, 0, None)
    assert rc == E_SHAPE and b"segments=0" in msg
    rc, msg = _call(-3, 64, None, None, None, 0, None)
    assert rc == E_SHAPE and b"segments=-3" in msg
    rc, msg = _call(1 << 30, 1 << 11, None, None, None, 0, None)      # 2^41 entries
    assert rc == E_UNSUPPORTED and b"2^40" in msg and b"seg_len=2048" in msg
    idx, adv, out, scr = _ptr(0x10000, L.c_i64_p), _ptr(0x20000, L.c_float_p), _ptr(0x30000, L.c_float_p), _ptr(0x40000, L.c_f64_p)
    for args in ((None, adv, out, scr), (idx, None, out, scr), (idx, adv, None, scr), (idx, adv, out, None)):
        rc, msg = _call(2, 64, args[0], args[1], args[2], 129, args[3])
        assert rc == E_BADARG and b"null pointer" in msg
    rc, msg = _call(2, 64, idx, adv, out, 127, scr)      # 128 distinct rows do not fit into 127
    assert rc == E_SHAPE and b"rows=127" in msg
    # out begins inside adv's rows (and the reverse); the columns of 129 floats are 516 bytes long
    for a, o in ((0x20000, 0x20000), (0x20000, 0x20000 + 4 * 128), (0x20000 + 4 * 128, 0x20000)):
        rc, msg = _call(2, 64, idx, _ptr(a, L.c_float_p), _ptr(o, L.c_float_p), 129, scr)
        assert rc == E_BADARG and b"overlap" in msg and b"rows=129" in msg
