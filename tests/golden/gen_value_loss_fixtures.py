#!/usr/bin/env python
"""Record the PPO-update fixtures of the UNCLIPPED value loss by running the reference itself (unmodified, on CPU) with
use_clipped_value_loss = False (algo/ppo/ppo.py:158-166: value_loss = (returns - value_batch).pow(2).mean()).

    python tests/golden/gen_value_loss_fixtures.py          (from the repository root)

Needs the reference checkout that gen_fixtures.py needs (ref_harness.load_reference).  Outputs (small, committed):
  tests/golden/ppo_update_unclipped.npz       gen_fixtures.gen_ppo_update's case (small widths), unclipped
  tests/golden/ppo_update_full_unclipped.npz  gen_fixtures.gen_ppo_update_full's case (XBot-L widths, ppo_full_case.py), unclipped
Both recorders are reused as they are: they receive the reference with its PPO constructor forced to use_clipped_value_loss =
False, and their np.savez_compressed is redirected here.  Everything up to the update must come out as in the clipped fixture
(asserted); of the rest the files keep what tests/golden/value_loss_case.py describes, written with fixed zip timestamps (so that
two runs give byte-identical files) together with use_clipped_value_loss = False.

In minibatch 0 of epoch 1 the stored values equal the current ones, so both value-loss forms give the same first gradient `g0`;
only the parameter change over all steps (`dP`), the losses and the learning rates can tell them apart.  The recorder prints, per
tensor, the rel-L2 distance between the unclipped and the clipped fixture's dP, and the two mean value losses."""
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fixtures as G  # noqa: E402
import ref_harness as H  # noqa: E402
import value_loss_case as V  # noqa: E402

RESULTS = ("lrs", "mean_value_loss", "mean_surrogate_loss", "final_lr")     # what the update computed (besides g0 / p1 / pF / dP)


def unclipped_reference(R):
    """The loaded reference with PPO(...) always built with use_clipped_value_loss = False."""
    ref_ppo = R.PPO

    def PPO(*a, **k):
        k["use_clipped_value_loss"] = False
        return ref_ppo(*a, **k)

    return types.SimpleNamespace(**dict(vars(R), PPO=PPO))


def savez_deterministic(path, arrays):
    """np.savez_compressed's layout (one .npy member per array, deflated) with a fixed member timestamp."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def record(gen, R):
    """Run one of gen_fixtures' recorders on the unclipped reference; returns every array it would have written."""
    captured = {}
    orig = np.savez_compressed

    def capture(path, **arrays):
        captured.update(arrays)

    np.savez_compressed = capture
    try:
        gen(unclipped_reference(R))
    finally:
        np.savez_compressed = orig
    return captured


def keep(u, name_c, name):
    """Check that u (a recorded unclipped case) shares everything up to the update with the clipped fixture name_c, and write what
    value_loss_case.py says the unclipped fixture keeps to `name`."""
    c = np.load(os.path.join(HERE, name_c))
    update = lambda k: k in RESULTS or k.startswith(("g0_", "p1_", "pF_", "dP_"))
    shared = sorted(k for k in u if not update(k))
    assert shared == sorted(k for k in c.files if not update(k)), (name, shared)
    for k in shared:
        assert np.array_equal(u[k], c[k]), (name, k)
    out = {k: u[k] for k in RESULTS}
    if "g0_s32_std" in u:       # full case: the recorder's fp32-exact samples, thinned, and the tensors' norms
        for n in V.NAMES:
            key = n.replace(".", "_")
            for prefix in ("g0", "dP"):
                out["%s_s32_%s" % (prefix, key)] = u["%s_s32_%s" % (prefix, key)][::V.STRIDE[prefix]]
                out["%s_norm_%s" % (prefix, key)] = u["%s_norm_%s" % (prefix, key)]
    else:                       # small case: whole tensors recorded, samples taken here
        for n in V.NAMES:
            key = n.replace(".", "_")
            for prefix in ("g0", "pF"):
                a = u["%s_%s" % (prefix, key)].reshape(-1)
                out["%s_s32_%s" % (prefix, key)] = a[V.sample_index(n, a.size, prefix)]
    out["use_clipped_value_loss"] = np.array(False)
    savez_deterministic(os.path.join(HERE, name), out)
    print("%s: %d bytes" % (name, os.path.getsize(os.path.join(HERE, name))))


def param_change(f, key):
    """dP of one tensor: pF - p0 (small fixture) or the full fixture's dP (fp16 x scale, or the fp32-exact whole tensor)."""
    if "pF_" + key in f:
        return (f["pF_" + key].astype(np.float64) - f["p0_" + key].astype(np.float64)).reshape(-1)
    if "dP_h16_" + key in f:
        return f["dP_h16_" + key].astype(np.float64).reshape(-1) / float(f["dP_h16_scale"])
    return f["dP_s32_" + key].astype(np.float64).reshape(-1)


def separation(name_u, u, name_c):
    c = dict(np.load(os.path.join(HERE, name_c)))
    keys = sorted({k[3:] for k in c if k.startswith("pF_")} | {k[len("dP_s32_"):] for k in c if k.startswith("dP_s32_")})
    print("%s vs %s: mean_value_loss %.9g (unclipped) vs %.9g (clipped); lrs %s vs %s" % (
        name_u, name_c, float(u["mean_value_loss"]), float(c["mean_value_loss"]), np.asarray(u["lrs"]).tolist(), np.asarray(c["lrs"]).tolist()))
    for k in keys:
        du, dc = param_change(u, k), param_change(c, k)
        print("  dP %-18s rel-L2 %.4e" % (k, np.linalg.norm(du - dc) / max(np.linalg.norm(dc), 1e-30)))


if __name__ == "__main__":
    R = H.load_reference()
    u = record(G.gen_ppo_update, R)
    uf = record(G.gen_ppo_update_full, R)
    keep(u, "ppo_update.npz", "ppo_update_unclipped.npz")
    keep(uf, "ppo_update_full.npz", "ppo_update_full_unclipped.npz")
    separation("ppo_update_unclipped.npz", u, "ppo_update.npz")
    separation("ppo_update_full_unclipped.npz", uf, "ppo_update_full.npz")
