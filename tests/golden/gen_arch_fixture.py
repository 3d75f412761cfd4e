#!/usr/bin/env python
"""Record one full reference PPO iteration (act -> bootstrap -> GAE -> 2 epochs x 4 minibatches) at an architecture unlike XBot-L's:
actor [37, 5], critic [100, 17, 65, 3], 141 observations, 73 privileged, 5 actions -- two and four hidden layers, ragged widths, a
head narrower than 12.

    python tests/golden/gen_arch_fixture.py          (from the repository root)

Needs the reference checkout that gen_fixtures.py needs (ref_harness.load_reference).  gen_fixtures.gen_ppo_update is reused as it
is, with these shapes; its np.savez_compressed is redirected so that the file is written with fixed zip timestamps (two runs give
byte-identical files).  Output (small, committed): tests/golden/ppo_update_arch.npz, the keys of ppo_update.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fixtures as G  # noqa: E402
import gen_value_loss_fixtures as VL  # noqa: E402
import ref_harness as H  # noqa: E402

NAME = "ppo_update_arch.npz"
SHAPE = dict(num_obs=141, num_priv=73, num_actions=5, actor_hidden=[37, 5], critic_hidden=[100, 17, 65, 3])


if __name__ == "__main__":
    R = H.load_reference()
    captured = {}
    orig = np.savez_compressed
    np.savez_compressed = lambda path, **arrays: captured.update(arrays)
    try:
        G.gen_ppo_update(R, name=NAME, **SHAPE)
    finally:
        np.savez_compressed = orig
    VL.savez_deterministic(os.path.join(HERE, NAME), captured)
    print("%s: %d bytes" % (NAME, os.path.getsize(os.path.join(HERE, NAME))))
