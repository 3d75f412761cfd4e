"""What tests/golden/ppo_update_unclipped.npz and ppo_update_full_unclipped.npz keep of the reference's PPO update with
use_clipped_value_loss = False, and where a replay finds the rest.

The two unclipped cases run on the inputs of the clipped fixtures (ppo_update.npz, ppo_update_full.npz + ppo_full_case.py): the same
seeds, initial parameters, rollout and minibatch permutation -- the value-loss form plays no part before the update, and the recorder
asserts that everything up to the update came out identical.  So the unclipped files hold only what the update computed: the learning
rates, the mean losses, and fp32-exact samples of the first minibatch's gradient (`g0`) and of the parameters after the update (small
case: `pF`) or of their change (full case: `dP`), plus the full tensors' norms (full case).  A sample of tensor `name` holds the
entries at sample_index(name, numel, prefix), a subset of the entries the clipped full-width fixture keeps exactly."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_full_case as CASE  # noqa: E402

STRIDE = {"g0": 8, "pF": 1, "dP": 1}        # every STRIDE-th entry of ppo_full_case.sample_index: <= 512 / 4096 / 4096 per tensor
NAMES = CASE.NAMES                          # the small case's tensors carry the same names


def sample_index(name, numel, prefix):
    """Flat indices of the entries of tensor `name` (numel entries) that the unclipped fixtures keep under `prefix`."""
    return CASE.sample_index(name, numel)[::STRIDE[prefix]]
