"""The unclipped value loss as a configuration choice (HgymPPOConfig.value_loss_unclipped), host side: the C layout, what
make_ppo_config writes, PPO's signature, and the reference fixtures recorded with use_clipped_value_loss = False
(tests/golden/gen_value_loss_fixtures.py) against the clipped ones."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

from hgym import _lib as L, make_ppo_config

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import value_loss_case as V  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAIRS = [("ppo_update_unclipped.npz", "ppo_update.npz"), ("ppo_update_full_unclipped.npz", "ppo_update_full.npz")]


def test_field_is_appended_to_the_ppo_config():
    assert L.PPOConfig._fields_[-1] == ("value_loss_unclipped", C.c_int32)
    assert C.sizeof(L.PPOConfig) == L.lib.hgym_sizeof(b"HgymPPOConfig")
    assert L.PPOConfig.value_loss_unclipped.offset == L.PPOConfig.grad_norm_ready.offset + 4


def test_make_ppo_config_sets_the_form():
    assert make_ppo_config().value_loss_unclipped == 0
    assert make_ppo_config(clipped_value_loss=True).value_loss_unclipped == 0
    assert make_ppo_config(clipped_value_loss=False).value_loss_unclipped == 1
    # the rest of the configuration does not depend on the form
    a, b = make_ppo_config(), make_ppo_config(clipped_value_loss=False)
    b.value_loss_unclipped = 0
    assert C.string_at(C.addressof(a), C.sizeof(a)) == C.string_at(C.addressof(b), C.sizeof(b))


def test_ppo_still_defaults_to_the_clipped_loss():
    from humanoid.algo import PPO
    assert inspect.signature(PPO.__init__).parameters["use_clipped_value_loss"].default is True


def _clipped_at(Cl, prefix, name, key, stride):
    """The clipped fixture's fp32 values at the entries the unclipped fixture keeps (value_loss_case.sample_index)."""
    if prefix + "_s32_" + key in Cl.files:         # full case: the same index set, thinned
        return Cl["%s_s32_%s" % (prefix, key)][::stride]
    a = Cl["%s_%s" % (prefix, key)].reshape(-1)   # small case: whole tensors
    return a[V.sample_index(name, a.size, prefix)]


@pytest.mark.parametrize("unclipped,clipped", PAIRS)
def test_unclipped_fixtures_against_the_clipped_ones(unclipped, clipped):
    U, Cl = np.load(os.path.join(GOLDEN, unclipped)), np.load(os.path.join(GOLDEN, clipped))
    assert bool(U["use_clipped_value_loss"]) is False
    assert os.path.getsize(os.path.join(GOLDEN, unclipped)) < 160 * 1024      # update results only: the inputs are the clipped fixture's
    after = "dP" if "dP_s32_std" in U.files else "pF"
    for name in V.NAMES:
        key = name.replace(".", "_")
        # minibatch 0 of epoch 1: the stored values are the current ones, so both forms give the same gradient
        a, b = U["g0_s32_" + key].astype(np.float64), _clipped_at(Cl, "g0", name, key, V.STRIDE["g0"]).astype(np.float64)
        assert a.shape == b.shape and a.size > 0, key
        assert np.abs(a - b).max() <= 1e-6 * max(np.abs(b).max(), 1e-30), key
        # ... after that they part: the critic's parameters end elsewhere
        a, b = U["%s_s32_%s" % (after, key)], _clipped_at(Cl, after, name, key, V.STRIDE[after])
        assert a.shape == b.shape
        if name.startswith("critic."):
            assert not np.array_equal(a, b), key
    assert float(U["mean_value_loss"]) != float(Cl["mean_value_loss"])
    assert U["lrs"].shape == Cl["lrs"].shape == (8,)
