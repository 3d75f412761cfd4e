"""CPU-only: the mirror loss of left-right symmetry (PPO.mirror_loss_coef, HgymPPOConfig.mirror_coef) -- the
plumbing from the train config to the C structs, mirror_pair_rows, and that the float64 reference of tests/mirror_loss_common.py can
see every way the term could be built wrong."""
import copy
import ctypes as C

import pytest
import torch

import hgym
from hgym import _lib as L
import mirror_loss_common as M
import update_options_common as U


# ------------------------------------------------------------------------------------------------ plumbing
def test_class_attribute_defaults():
    from humanoid.algo import PPO
    assert PPO.mirror_loss_coef == 0.0 and PPO.symmetry_augmentation is True and PPO.symmetry is None


NATIVE = [({}, (False, 0.0)), ({"symmetry": True}, (True, 0.0)), ({"symmetry": True, "symmetry_augmentation": False}, (False, 0.0)),
          ({"mirror_loss_coef": 0.25}, (False, 0.25)), ({"symmetry": True, "mirror_loss_coef": 0.25}, (True, 0.25)),
          ({"symmetry": True, "symmetry_augmentation": False, "mirror_loss_coef": 2.0}, (False, 2.0))]
RSL = [({"symmetry_cfg": dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.5)}, (True, 0.0)),
       ({"symmetry_cfg": dict(use_data_augmentation=False, use_mirror_loss=True, mirror_loss_coeff=0.5)}, (False, 0.5)),
       ({"symmetry_cfg": dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=1.5)}, (True, 1.5)),
       ({"symmetry_cfg": dict(use_mirror_loss=True, mirror_loss_coeff=1.5), "symmetry": True}, (True, 1.5))]


@pytest.mark.parametrize("block, want", NATIVE + RSL)
def test_both_config_spellings(block, want):
    from humanoid.algo.ppo.on_policy_runner import _split_algorithm_cfg, _split_symmetry_cfg
    cfg = dict(clip_param=0.2, num_mini_batches=4, **block)
    before = copy.deepcopy(cfg)
    kwargs, symmetry = _split_algorithm_cfg(cfg)
    got = _split_symmetry_cfg(cfg)
    assert cfg == before                                         # the caller's dict is left alone
    assert kwargs == dict(clip_param=0.2, num_mini_batches=4)      # none of the native keys reaches PPO.__init__
    assert symmetry is bool(block.get("symmetry", False))        # the meaning tests/test_symmetry.py pins
    assert got == want and isinstance(got[0], bool) and isinstance(got[1], float)


def test_spellings_that_disagree_are_refused():
    from humanoid.algo.ppo.on_policy_runner import _split_symmetry_cfg
    with pytest.raises(ValueError):
        _split_symmetry_cfg({"mirror_loss_coef": 0.25, "symmetry_cfg": dict(use_mirror_loss=True, mirror_loss_coeff=0.5)})
    with pytest.raises(ValueError):
        _split_symmetry_cfg({"symmetry": False, "symmetry_cfg": dict(use_data_augmentation=True)})
    with pytest.raises(ValueError):
        _split_symmetry_cfg({"symmetry_cfg": dict(use_mirror_los=True)})


def test_make_ppo_config_writes_the_field_and_a_zero_tail_is_off():
    p = hgym.make_ppo_config(mirror_coef=0.375)
    assert p.mirror_coef == 0.375
    off = hgym.make_ppo_config()
    assert off.mirror_coef == 0.0
    # appended at the tail: every earlier field sits where it sat (tests/test_value_loss.py pins the last of them), the new one lies
    # right behind, and it is what the library reads there
    at = L.MIRROR_COEF_OFFSET
    assert at == L.PPOConfig.value_loss_unclipped.offset + 4 and at + 4 == C.sizeof(L.PPOConfig)
    import struct
    raw = lambda c: bytes(C.string_at(C.addressof(c), C.sizeof(c)))
    assert raw(p)[at:] == struct.pack("<f", 0.375) and raw(p)[:at] == raw(off)[:at]
    assert raw(off)[at:] == bytes(4)
    assert [f[0] for f in L.Batch._fields_][-6:] == ["num_rows", "pair_idx", "mirror_act_src", "mirror_act_sign", "mirror_target", "mirror_sums"]
    b = L.Batch()
    assert not b.pair_idx and not b.mirror_act_src and not b.mirror_act_sign and not b.mirror_target and not b.mirror_sums


def test_sizeof_equals_the_ctypes_mirrors():
    for name in ("HgymPPOConfig", "HgymBatch"):
        assert int(L.lib.hgym_sizeof(name.encode())) == C.sizeof(L.STRUCTS[name]), name
    assert C.sizeof(L.Batch) == 112 + 5 * 8


def test_make_batch_takes_the_pair_and_the_mirror_block():
    S, Bn, A = 6, 4, 3
    f = lambda *s: torch.zeros(*s)
    cols = [f(S, 5), f(S, 2), f(S, A), f(S), f(S), f(S), f(S), f(S, A), f(S, A)]
    idx, pair = torch.arange(Bn), torch.arange(Bn) + 1
    mirror = (torch.zeros(A, dtype=torch.int32), torch.ones(A), torch.zeros(Bn * A), torch.zeros(2, dtype=torch.float64))
    b = hgym.make_batch(*cols, idx, pair_idx=pair, mirror=mirror)
    addr = lambda p: C.cast(p, C.c_void_p).value
    assert addr(b.pair_idx) == pair.data_ptr() and addr(b.mirror_act_src) == mirror[0].data_ptr() and addr(b.mirror_act_sign) == mirror[1].data_ptr()
    assert addr(b.mirror_target) == mirror[2].data_ptr() and addr(b.mirror_sums) == mirror[3].data_ptr() and b.B == Bn
    plain = hgym.make_batch(*cols, idx)
    assert not plain.pair_idx and not plain.mirror_sums
    with pytest.raises(AssertionError):
        hgym.make_batch(*cols, idx, pair_idx=pair)


# ------------------------------------------------------------------------------------------------ mirror_pair_rows
def test_mirror_pair_rows():
    from humanoid.algo.ppo.rollout_storage import mirror_pair_rows
    T, N = 3, 5
    rows = torch.cat((torch.arange(T * N), torch.arange((T + 1) * N, (2 * T + 1) * N)))      # every row but the bootstrap slot's
    p = mirror_pair_rows(rows, T, N)
    assert p.dtype == torch.int64 and p.shape == rows.shape
    assert torch.equal(mirror_pair_rows(p, T, N), rows)                                        # an involution
    r = torch.arange(T * N)
    assert torch.equal(p[:T * N], (T + 1) * N + r) and torch.equal(p[T * N:], r)              # r <-> (T + 1) N + r
    assert not bool(((p >= T * N) & (p < (T + 1) * N)).any())                                  # never the bootstrap slot
    assert sorted(p.tolist()) == sorted(rows.tolist())


# ------------------------------------------------------------------------------------------------ the reference can see the feature
def _case(path):
    return M.case_of(U.Options(path, None, "scalar", False, False, False, False))


def _moved(case, a, b):
    e = U.errors(case["opts"], {k: g for k, g in a["grads"].items() if k.startswith("actor.")}, b,
                 names=[k for k in b["grads"] if k.startswith("actor.")])
    return max(e.values()) / U.bar_of(case["opts"])


@pytest.mark.parametrize("path", U.PATHS)
def test_reference_sees_every_way_to_build_the_term_wrong(path):
    """At the path's U.SHAPES and coefficient M.COEF = 0.5 (the first value tried; it holds all four), some ACTOR tensor moves by more than
    U.SENSITIVITY x its bar when (a) the term is dropped, (b) the target is not detached, (c) the identity table replaces MirrorSpec's
    action table, (d) the scale is 1 / B instead of 1 / (B A).  The nets are random, far from symmetric: |mu - t| is of the size of mu."""
    case = _case(path)
    assert M.COEF == 0.5
    ref = M.reference(case)
    A = len(case["spec"].act_src)
    assert ref["mirror"] > 0.1 * float((ref["mu"] ** 2).mean())      # not a nearly symmetric net
    wrong = dict(a_off=M.reference(case, coef=0.0), b_not_detached=M.reference(case, detach=False),
                 c_identity_table=M.reference(case, table=(list(range(A)), [1] * A)), d_one_over_B=M.reference(case, per_action=False))
    for name, w in wrong.items():
        moved = _moved(case, w, ref)
        print("%s %s: worst actor tensor moved %.1f bars" % (path, name, moved))
        assert moved > U.SENSITIVITY, (path, name, moved)
    off = U.reference(case["opts"], case["params"], case["stats"], case["cols"], case["idx"], case["ppo"])
    for k, g in off["grads"].items():      # coefficient 0 is update_options_common's reference itself; the term moves the actor only
        assert torch.equal(g, wrong["a_off"]["grads"][k]), k
        if not k.startswith("actor."):
            assert torch.equal(g, ref["grads"][k]), k
    for k in ("surrogate", "value", "entropy", "kl"):
        assert float(off["sums"][k]) == float(ref["sums"][k])
