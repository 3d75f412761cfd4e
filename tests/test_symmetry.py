"""CPU-only: the left-right mirror tables (humanoid/utils/symmetry.py) -- MirrorSpec's validation, XBot-L's tables against segment
tables composed here from the frame layout, the oracle's gait clock (half a cycle on = the mirrored gait), the joint signs against
zero-pose forward kinematics of the recorded leg chains, and the runner's filtering of the native `symmetry` key."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from humanoid.utils.symmetry import MirrorSpec, xbot_l_mirror

ID1 = ([0], [1])


def _cfg(frame_stack=15, c_frame_stack=3, single=47, single_priv=73, heights=False):
    return SimpleNamespace(env=SimpleNamespace(frame_stack=frame_stack, c_frame_stack=c_frame_stack, num_single_obs=single,
                                               single_num_privileged_obs=single_priv, num_actions=12),
                           terrain=SimpleNamespace(measure_heights=heights))


# ---------------------------------------------------------------------------------------------- MirrorSpec
@pytest.mark.parametrize("src, sign, column", [
    ([0, 1, 1], [1, 1, 1], 2),            # not a permutation
    ([0, 3, 1], [1, 1, 1], 1),            # a source outside the row
    ([1, 0, 2], [1, 1, 0], 2),            # a sign of 0
    ([1, 2, 0], [1, 1, 1], 0),            # a 3-cycle
    ([1, 0, 2], [1, -1, 1], 0),           # a swap with unequal signs
])
def test_mirror_spec_rejects_what_is_no_signed_involution(src, sign, column):
    for slot in range(3):
        tables = [ID1, ID1, ID1]
        tables[slot] = (src, sign)
        with pytest.raises(ValueError, match=r"column(s)? %d\b" % column):
            MirrorSpec(*tables[0], *tables[1], *tables[2])


def test_mirror_spec_accepts_signed_involutions_and_compares_by_content():
    a = MirrorSpec([1, 0, 2], [-1, -1, 1], [0], [-1], np.array([1, 0]), torch.tensor([1.0, 1.0]))
    b = MirrorSpec([1, 0, 2], [-1, -1, 1], [0], [-1], [1, 0], [1, 1])
    assert a == b and a.key() == b.key() and hash(a) == hash(b)
    assert a != MirrorSpec([1, 0, 2], [1, 1, 1], [0], [-1], [1, 0], [1, 1])


# ---------------------------------------------------------------------------------------------- XBot-L's tables
def _compose(widths, parts):
    """Segment tables -> one frame's (src, sign); parts[i] is (relative src, sign) of a segment widths[i] wide."""
    src, sign, base = [], [], 0
    for w, (s, g) in zip(widths, parts):
        assert len(s) == w and len(g) == w
        src += [base + x for x in s]
        sign += g
        base += w
    return src, sign


def _expected_frames():
    joint = ([6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5], [-1] * 12)
    keep = lambda *g: (list(range(len(g))), list(g))
    head = keep(-1, -1, 1, -1, -1)
    ang, lin, swap = keep(-1, 1, -1), keep(1, -1, 1), ([1, 0], [1, 1])
    obs = _compose((5, 12, 12, 12, 3, 3), (head, joint, joint, joint, ang, ang))
    priv = _compose((5, 12, 12, 12, 12, 3, 3, 3, 2, 3, 1, 1, 2, 2),
                    (head, joint, joint, joint, joint, lin, ang, ang, keep(1, -1), ang, keep(1), keep(1), swap, swap))
    return obs, priv, joint


def test_xbot_l_tables_equal_the_segment_tables_tiled():
    (osrc, osign), (psrc, psign), (asrc, asign) = _expected_frames()
    spec = xbot_l_mirror(_cfg())
    assert spec.obs_src == [f * 47 + s for f in range(15) for s in osrc] and spec.obs_sign == osign * 15
    assert spec.priv_src == [f * 73 + s for f in range(3) for s in psrc] and spec.priv_sign == psign * 3
    assert spec.act_src == asrc and spec.act_sign == asign
    assert len(spec.obs_src) == 705 and len(spec.priv_src) == 219
    small = xbot_l_mirror(_cfg(frame_stack=2, c_frame_stack=1))
    assert small.obs_src == osrc + [47 + s for s in osrc] and small.priv_src == psrc


def test_xbot_l_tables_match_the_registered_task_config():
    from humanoid.envs import task_registry      # noqa: F401  (registers humanoid_ppo)
    from humanoid.utils import task_registry as reg
    env_cfg, _ = reg.get_cfgs("humanoid_ppo")
    spec = xbot_l_mirror(env_cfg)
    assert len(spec.obs_src) == env_cfg.env.num_observations and len(spec.priv_src) == env_cfg.env.num_privileged_obs


@pytest.mark.parametrize("cfg", [_cfg(single=48), _cfg(single_priv=74), _cfg(heights=True)])
def test_xbot_l_mirror_refuses_other_layouts(cfg):
    with pytest.raises(NotImplementedError):
        xbot_l_mirror(cfg)


# ---------------------------------------------------------------------------------------------- the oracle's gait
def test_half_a_gait_cycle_on_is_the_mirrored_gait():
    """The cycle is 64 steps (cycle_time 0.64 s at dt 0.01): the reference pose and the stance mask at k + 32 are the mirror images of
    those at k -- what the table does to the clock columns (sin, cos -> -sin, -cos) and to the joint and stance columns is one
    consistent reflection.  The |sin| nearest the 0.1 threshold is 0.0980 at k = 1, 2e-3 away: fp32 cannot flip a mask."""
    from oracle.xbot_env_oracle import XBotEnvOracle
    spec = xbot_l_mirror(_cfg())
    o = XBotEnvOracle(64)
    o.ep_len = torch.arange(64)
    ref0, mask0 = o._ref_pose().clone(), o._stance_mask().clone()
    o.ep_len = torch.arange(64) + 32
    ref1, mask1 = o._ref_pose(), o._stance_mask()
    src, sign = torch.tensor(spec.act_src), torch.tensor(spec.act_sign, dtype=torch.float32)
    assert float(ref0.abs().max()) > 0.1
    assert float((ref1 - sign * ref0[:, src]).abs().max()) <= 1e-5
    assert torch.equal(mask1, mask0[:, [1, 0]])
    assert 0 < int((mask0[:, 0] != mask0[:, 1]).sum()) < 64


# ---------------------------------------------------------------------------------------------- joint signs from the robot description
def _rot_rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return rz @ ry @ rx      # URDF: fixed-axis roll, pitch, yaw


def _zero_pose_axes(chain):
    """{joint name: (axis in the base frame, joint origin in the base frame)} at the zero pose."""
    R, t, out = np.eye(3), np.zeros(3), {}
    for j in chain:
        t = t + R @ np.array(j["xyz"])
        R = R @ _rot_rpy(*j["rpy"])
        out[j["name"]] = (R @ np.array(j["axis"]), t.copy())
    return out


def test_joint_signs_follow_from_the_leg_chains(golden_dir):
    d = json.load(open(os.path.join(golden_dir, "xbot_l_leg_joints.json")))
    spec = xbot_l_mirror(_cfg())
    order = d["dof_order"]
    assert len(order) == 12 and all(n.startswith("left_") for n in order[:6]) and all(n.startswith("right_") for n in order[6:])
    left, right = _zero_pose_axes(d["chains"]["left"]), _zero_pose_axes(d["chains"]["right"])
    lim = {j["name"]: (j["lower"], j["upper"]) for side in ("left", "right") for j in d["chains"][side]}
    P = np.diag([1.0, -1.0, 1.0])      # the reflection through the sagittal plane (x forward, y left)
    assert left[order[0]][1][1] == pytest.approx(0.117, abs=1e-3) and right[order[6]][1][1] == pytest.approx(-0.117, abs=1e-3)
    for j in range(6):
        nl, nr = order[j], order[j + 6]
        assert nr == "right_" + nl[len("left_"):] and spec.act_src[j] == j + 6 and spec.act_src[j + 6] == j
        (al, tl), (ar, tr) = left[nl], right[nr]
        assert np.allclose(P @ tl, tr, atol=1e-3), (nl, tl, tr)        # the joints themselves are mirror images
        # a rotation by q about a_L mirrors to a rotation by q about the axial image -P a_L: the right joint's angle is q * (-P a_L) . a_R
        s = float(-(P @ al) @ ar)
        assert abs(s - spec.act_sign[j]) <= 1e-3 and abs(s - spec.act_sign[j + 6]) <= 1e-3, (nl, s)
        # ... and the limits negate and swap with it
        assert lim[nr] == (-lim[nl][1], -lim[nl][0]), (nl, lim[nl], lim[nr])


# ---------------------------------------------------------------------------------------------- runner plumbing
@pytest.mark.parametrize("block, on", [({}, False), ({"symmetry": False}, False), ({"symmetry": True}, True)])
def test_runner_takes_the_symmetry_key_out_of_the_algorithm_block(block, on):
    import inspect
    from humanoid.algo.ppo.on_policy_runner import _split_algorithm_cfg
    from humanoid.algo import PPO
    cfg = dict(dict(clip_param=0.2, num_mini_batches=4, learning_rate=1e-5), **block)
    before = dict(cfg)
    kwargs, symmetry = _split_algorithm_cfg(cfg)
    assert symmetry is on and "symmetry" not in kwargs and cfg == before        # (the caller's dict is left alone)
    assert kwargs == {k: v for k, v in cfg.items() if k != "symmetry"}
    assert set(kwargs) <= set(inspect.signature(PPO.__init__).parameters)
    assert PPO.symmetry is None
