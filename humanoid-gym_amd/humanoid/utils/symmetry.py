"""Left-right symmetry of the robot as column tables (PPO.symmetry).

Reflecting the scene through the robot's sagittal plane maps every observation, privileged observation and action vector to
another valid one: out[c] = sign[c] * in[src[c]].  A MirrorSpec holds the three tables; xbot_l_mirror builds XBot-L's from the
per-frame layout of humanoid_env.py's compute_observations.  Host data only (lists of ints): the rollout storage puts them on the
device (RolloutStorage.enable_mirror)."""

NUM_DOF = 12
OBS_FRAME = 47
PRIV_FRAME = 73


def _validate(name, src, sign):
    w = len(src)
    if w < 1 or len(sign) != w:
        raise ValueError("%s: %d source columns, %d signs" % (name, w, len(sign)))
    seen = [False] * w
    for c, s in enumerate(src):
        if not (isinstance(s, int) and 0 <= s < w):
            raise ValueError("%s: column %d names source column %r outside [0, %d)" % (name, c, s, w))
        if seen[s]:
            raise ValueError("%s: not a permutation -- column %d names source column %d a second time" % (name, c, s))
        seen[s] = True
    for c, g in enumerate(sign):
        if g not in (1, -1):
            raise ValueError("%s: sign %r of column %d is neither +1 nor -1" % (name, g, c))
    for c in range(w):
        if src[src[c]] != c:
            raise ValueError("%s: not an involution -- column %d comes from %d, which comes from %d" % (name, c, src[c], src[src[c]]))
        if sign[c] * sign[src[c]] != 1:
            raise ValueError("%s: not an involution -- columns %d and %d swap with unequal signs" % (name, c, src[c]))


def _ints(v):
    v = v.tolist() if hasattr(v, "tolist") else list(v)
    return [int(x) if float(x) == int(x) else x for x in v]


class MirrorSpec:
    """Three tables (src, sign), out[c] = sign[c] * in[src[c]]: observations, privileged observations, actions (the action table also
    serves mu; sigma takes its permutation with sign +1).  Each must be a signed involution -- a permutation with src[src[c]] == c and
    sign[c] * sign[src[c]] == 1, sign in {+1, -1} -- because mirroring twice is the identity; ValueError names the first offending column."""

    def __init__(self, obs_src, obs_sign, priv_src, priv_sign, act_src, act_sign):
        self.obs_src, self.obs_sign = _ints(obs_src), _ints(obs_sign)
        self.priv_src, self.priv_sign = _ints(priv_src), _ints(priv_sign)
        self.act_src, self.act_sign = _ints(act_src), _ints(act_sign)
        _validate("obs", self.obs_src, self.obs_sign)
        _validate("priv", self.priv_src, self.priv_sign)
        _validate("act", self.act_src, self.act_sign)

    def key(self):
        """Hashable contents (PPO.update_graph_key)."""
        return tuple(tuple(t) for t in (self.obs_src, self.obs_sign, self.priv_src, self.priv_sign, self.act_src, self.act_sign))

    def __eq__(self, other):
        return isinstance(other, MirrorSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())


def _segments(*parts):
    """Concatenate per-segment tables: each part is (src relative to the segment, sign)."""
    src, sign = [], []
    for s, g in parts:
        base = len(sign)
        src += [base + x for x in s]
        sign += list(g)
    return src, sign


def _keep(signs):
    return list(range(len(signs))), list(signs)


_JOINTS = ([(j + NUM_DOF // 2) % NUM_DOF for j in range(NUM_DOF)], [-1] * NUM_DOF)      # legs swapped, every joint negated
_CLOCK_CMD = _keep([-1, -1, +1, -1, -1])      # sin, cos of the gait phase (half a cycle on); vx, vy, yaw-rate command
_ANG = _keep([-1, +1, -1])                    # a pseudo-vector (angular velocity, Euler angles, torque): roll, pitch, yaw
_LIN = _keep([+1, -1, +1])                    # a vector: x, y, z
_SWAP2 = ([1, 0], [+1, +1])                   # (left, right) flags


def xbot_l_frames():
    """(obs_src, obs_sign), (priv_src, priv_sign), (act_src, act_sign) of ONE frame: 47 / 73 / 12 columns."""
    obs = _segments(_CLOCK_CMD, _JOINTS, _JOINTS, _JOINTS, _ANG, _ANG)                        # phase + commands | q | dq | actions | omega | euler
    priv = _segments(_CLOCK_CMD, _JOINTS, _JOINTS, _JOINTS, _JOINTS, _LIN, _ANG, _ANG,        # ... | diff | v | omega | euler
                     _keep([+1, -1]), _ANG, _keep([+1]), _keep([+1]), _SWAP2, _SWAP2)         # push force xy | push torque | friction | mass | stance | contact
    assert len(obs[0]) == OBS_FRAME and len(priv[0]) == PRIV_FRAME
    return obs, priv, (list(_JOINTS[0]), list(_JOINTS[1]))


def _tile(table, frames, width):
    src, sign = table
    return [f * width + s for f in range(frames) for s in src], list(sign) * frames


def xbot_l_mirror(env_cfg):
    """The MirrorSpec of XBot-L's observation layout (humanoid_env.py: compute_observations) for env_cfg.env.frame_stack /
    c_frame_stack stacked frames.  NotImplementedError for another frame layout (num_single_obs != 47, single_num_privileged_obs != 73)
    and for terrain-height observations (terrain.measure_heights), whose columns this table does not describe."""
    e = env_cfg.env
    if int(e.num_single_obs) != OBS_FRAME or int(e.single_num_privileged_obs) != PRIV_FRAME:
        raise NotImplementedError("xbot_l_mirror describes frames of %d / %d columns, not %d / %d"
                                  % (OBS_FRAME, PRIV_FRAME, int(e.num_single_obs), int(e.single_num_privileged_obs)))
    if getattr(getattr(env_cfg, "terrain", None), "measure_heights", False):
        raise NotImplementedError("xbot_l_mirror: terrain-height observations (terrain.measure_heights) are not covered")
    if int(getattr(e, "num_actions", NUM_DOF)) != NUM_DOF:
        raise NotImplementedError("xbot_l_mirror: %d actions, not %d" % (int(e.num_actions), NUM_DOF))
    obs, priv, act = xbot_l_frames()
    return MirrorSpec(*_tile(obs, int(e.frame_stack), OBS_FRAME), *_tile(priv, int(e.c_frame_stack), PRIV_FRAME), *act)
