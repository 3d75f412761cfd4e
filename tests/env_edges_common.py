"""Planted-input edge suite for the env step: one env per case, each case on one side of one branch of the per-env chain.

The trace tests (env_common.run_random_trace, synth_common, the golden traces) draw ordinary states, and ordinary states never
reach several of the branches the step takes: the upper clamp of feet_contact_forces, the observation clip, the gimbal branch of
the Euler conversion, an operand exactly ON a threshold.  Here every such edge is PLANTED: a table of cases (CASES), each a name,
the edge it targets and a function that overwrites one env's pre-step state / sim frame / noise draws, batched together with
ordinary filler envs (env_common.synth_frames) at shuffled positions so that a workgroup holds a mixture and tiles are ragged.

Two references judge one post-physics step:
  * the fp32 oracle (oracle/xbot_env_oracle.py), to the project's bars (env_common.RTOL / ATOL, the torque floor), per reward term:
    the episode sums are zeroed before the step, so after it they ARE the terms times their scale (non-resetting envs);
  * `ref64_step` below: the same step restated in float64 from the reference's formulas (humanoid_env.py / legged_robot.py lines
    cited per block), every fp32 input widened exactly.  A python double the reference applies to an fp32 tensor is rounded to
    fp32 first by torch, so the constants here are F(x) = the double that equals fp32(x): thresholds sit where the reference's do.
    Nobody had measured how far the fp32 oracle itself is from this; build() measures it per term and per state field over the
    table (in units of the fp32 bar) and the product is allowed max(fp32 bar, 4 x that distance): a different summation order
    and the hardware exp2 / sqrt / sin / cos are about one ulp each (hgym_env_math.hpp, comment above r_exp).

Three passes, because some edges are properties of the configuration or of the common step counter, not of an env:
  ones      every reward scale 1 (each term visible at its own magnitude), counter on the push interval;
  default   the XBot-L scales, counter one before the push interval, only_positive_rewards on;
  signed    the XBot-L scales, only_positive_rewards off, and a cycle_time for which episode length 5 puts sin(phase) EXACTLY on
            0.1f (the double-stance test is `< 0.1`; with cycle_time 0.64 no integer episode length lands on it).
build() asserts the census: for every named edge, how many cases land on each side, counted from the float64 reference; a side
with no case fails, so a renamed constant or a changed default cannot quietly turn an edge case into an ordinary one.  It also
asserts, per case, that the fp32 oracle and the float64 reference take the same side of every predicate (a case where they do
not is a badly built case: move it away from the threshold).  No case is dropped at run time; the table's length is asserted.
"""
import math

import numpy as np
import torch

import env_common as EC
from oracle import xbot_constants as K
from oracle.xbot_env_oracle import XBotEnvOracle
from hgym import _lib as L

F = lambda x: float(np.float32(x))
FEET, KNEES, BASE = list(K.FEET_BODIES), list(K.KNEE_BODIES), K.BASE_BODY
NUM_CASES = 99
# With this cycle_time and episode length 5 the fp32 argument of the gait sine, fp32(2 pi) * (5 * fp32(0.01) / fp32(CYCLE_EXACT)) rounded
# after each operation, has an exact sine of 0.1f + 0.11 ulp: every sinf good to 0.39 ulp there returns 0.1f itself (glibc's and
# torch's do).  The float64 reference, which does not round the argument, gets 0.1f + 0.65 ulp: the same side of `< 0.1f`.  Found by
# a search over the fp32 neighbours of ep * 0.01 / (asin(0.1) / 2 pi), ep = 1 .. 8; no cycle_time near 0.64 has both properties.
CYCLE_EXACT = float(np.float32(3.1363415718078613))
PASSES = {
    "ones": dict(scales=[1.0] * K.NUM_REWARDS, only_positive=True, csc=K.PUSH_INTERVAL - 1, cycle_time=K.CYCLE_TIME),
    "default": dict(scales=list(K.REWARD_SCALES_DT), only_positive=True, csc=K.PUSH_INTERVAL - 2, cycle_time=K.CYCLE_TIME),
    "signed": dict(scales=list(K.REWARD_SCALES_DT), only_positive=False, csc=K.PUSH_INTERVAL - 2, cycle_time=CYCLE_EXACT),
}
STATE_FIELDS = ("commands", "actions", "last_actions", "last_last_actions", "last_dof_vel", "last_root_vel", "feet_air_time",
                "feet_height", "last_feet_z", "ref_dof_pos", "push_force", "push_torque", "episode_sums")
up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
dn = lambda x: float(np.nextafter(np.float32(x), np.float32(-np.inf)))


# ------------------------------------------------------------------------------------------------ the float64 reference
def _rot_inv(q, v):
    """isaacgym.torch_utils.quat_rotate_inverse, xyzw (call sites legged_robot.py:133-135)."""
    w, u = q[:, 3:4], q[:, :3]
    return v * (2.0 * w ** 2 - 1.0) - np.cross(u, v) * w * 2.0 + u * np.sum(u * v, axis=1, keepdims=True) * 2.0


def _rot(q, v):
    """isaacgym.torch_utils.quat_apply (call site legged_robot.py:312)."""
    u = q[:, :3]
    t = np.cross(u, v) * 2.0
    return v + q[:, 3:4] * t + np.cross(u, t)


def _euler(q):
    """get_euler_xyz, each angle % 2 pi, then the (-pi, pi] fold of legged_robot.py:50-55."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    roll = np.arctan2(2.0 * (w * x + y * z), w * w - x * x - y * y + z * z)
    sp = 2.0 * (w * y - z * x)
    gimbal = np.abs(sp) >= 1.0
    pitch = np.where(gimbal, np.sign(sp) * F(math.pi / 2.0), np.arcsin(np.clip(sp, -1.0, 1.0)))
    yaw = np.arctan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z)
    e = np.mod(np.stack((roll, pitch, yaw), axis=1), F(2 * math.pi))
    return np.where(e > F(math.pi), e - F(2 * math.pi), e), sp


def _sin_phase(ep, cycle_time):
    """humanoid_env.py:100-108."""
    phase = ep.astype(np.float64) * F(K.DT) / F(cycle_time)
    return np.sin(F(2 * math.pi) * phase), np.cos(F(2 * math.pi) * phase)


def _stance(s):
    """humanoid_env.py:105-118."""
    m = np.stack((s >= 0, s < 0), axis=1).astype(np.float64)
    m[np.abs(s) < F(0.1)] = 1.0
    return m


def _ref_pose(s):
    """humanoid_env.py:121-142."""
    sl, sr = np.where(s > 0, 0.0, s), np.where(s < 0, 0.0, s)
    s1 = F(K.TARGET_JOINT_POS_SCALE)
    ref = np.zeros((s.shape[0], 12))
    ref[:, 2], ref[:, 3], ref[:, 4] = sl * s1, sl * (2 * s1), sl * s1
    ref[:, 8], ref[:, 9], ref[:, 10] = sr * s1, sr * (2 * s1), sr * s1
    ref[np.abs(s) < F(0.1)] = 0.0
    return ref


def _resample(cmd, m, u3):
    """legged_robot.py:322-336 (heading command)."""
    rng = lambda r, u: F(r[1] - r[0]) * u + F(r[0])
    cmd = cmd.copy()
    cmd[:, 0] = np.where(m, rng(K.CMD_LIN_VEL_X, u3[:, 0]), cmd[:, 0])
    cmd[:, 1] = np.where(m, rng(K.CMD_LIN_VEL_Y, u3[:, 1]), cmd[:, 1])
    cmd[:, 3] = np.where(m, rng(K.CMD_HEADING, u3[:, 2]), cmd[:, 3])
    norm = np.sqrt(cmd[:, 0] ** 2 + cmd[:, 1] ** 2)
    keep = norm > F(0.2)
    cmd[:, :2] = np.where(m[:, None], cmd[:, :2] * keep[:, None], cmd[:, :2])
    return cmd, norm


def _dist_term(xy, max_df):
    """humanoid_env.py:282-305."""
    d = np.sqrt(np.sum((xy[:, 0] - xy[:, 1]) ** 2, axis=1))
    d_min = np.clip(d - F(K.MIN_DIST), -0.5, 0.0)      # (the lower bound -0.5 cannot bind: d >= 0 > MIN_DIST - 0.5)
    d_max = np.clip(d - F(max_df), 0.0, 0.5)
    return (np.exp(-np.abs(d_min) * 100) + np.exp(-np.abs(d_max) * 100)) / 2, d


def ref64_pre(S, a_in, u_delay, z_act):
    """humanoid_env.py:189-197 + legged_robot.py:90-91 (action filter) and legged_robot.py:340-356 (PD torques), float64."""
    clip = F(K.CLIP_ACTIONS)
    a = np.clip(a_in, -clip, clip)
    delay = u_delay[:, None] * F(K.ACTION_DELAY)
    a = (1 - delay) * a + delay * S["actions"]
    a = a + F(K.ACTION_NOISE) * z_act * a
    act = np.clip(a, -clip, clip)
    lim = np.array([F(e * K.TORQUE_LIMIT_FACTOR) for e in K.EFFORT])
    raw = np.array(K.P_GAINS) * (act * F(K.ACTION_SCALE) + np.array(K.DEFAULT_DOF_POS) - S["pre_dof_pos"]) - np.array(K.D_GAINS) * S["pre_dof_vel"]
    return act, np.clip(raw, -lim, lim), dict(a_hi=(a_in > clip).any(1), a_lo=(a_in < -clip).any(1), a2_clip=(np.abs(a) > clip).any(1),
                                              tq_hi=(raw > lim).any(1), tq_lo=(raw < -lim).any(1), tq_in=(np.abs(raw) < lim).all(1))


def ref64_step(S, cfg):
    """One LeggedRobot.post_physics_step (legged_robot.py:119-151) with XBotLFreeEnv's rewards (humanoid_env.py:272-540) in float64.
    S: every input as float64 / int64 numpy arrays (fp32 values widened exactly); cfg: a PASSES entry.  Returns the outputs and `pred`,
    which side of each predicate every env took."""
    N = S["ep_len"].shape[0]
    dt, ct = F(K.DT), cfg["cycle_time"]
    pred = {}
    ep = S["ep_len"] + 1                                                    # legged_robot.py:128-129
    csc = cfg["csc"] + 1
    root, q = S["root"].copy(), S["root"][:, 3:7]
    blv, bav = _rot_inv(q, root[:, 7:10]), _rot_inv(q, root[:, 10:13])      # :132-136
    grav = _rot_inv(q, np.tile([0.0, 0.0, -1.0], (N, 1)))
    eul, sp = _euler(q)
    pred["sp"] = sp
    # _post_physics_step_callback :304-320
    resample = ep % K.RESAMPLE_STEPS == 0
    cmd, norm = _resample(S["commands"], resample, S["u_cmd"][:, 0:3])
    pred["resample"], pred["cmd_norm"] = resample, norm
    fwd = _rot(q, np.tile([1.0, 0.0, 0.0], (N, 1)))
    ang0 = cmd[:, 3] - np.arctan2(fwd[:, 1], fwd[:, 0])
    ang = np.mod(ang0, F(2 * math.pi))                                      # utils/math.py:46-49
    ang = ang - F(2 * math.pi) * (ang > F(math.pi))
    cmd[:, 2] = np.clip(0.5 * ang, -1.0, 1.0)
    pred["heading_diff"], pred["half_ang"] = ang0, 0.5 * ang
    pf, pt = S["push_force"].copy(), S["push_torque"].copy()
    pushed = csc % K.PUSH_INTERVAL == 0                                     # humanoid_env.py:83-98
    if pushed:
        pf[:, :2] = F(2 * K.MAX_PUSH_VEL_XY) * S["u_push"][:, 0:2] + F(-K.MAX_PUSH_VEL_XY)
        pt = F(2 * K.MAX_PUSH_ANG_VEL) * S["u_push"][:, 2:5] + F(-K.MAX_PUSH_ANG_VEL)
        root[:, 7:9], root[:, 10:13] = pf[:, :2], pt
    pred["pushed"] = np.full(N, pushed)
    # check_termination :156-161
    bn = np.sqrt(np.sum(S["contact"][:, BASE] ** 2, axis=1))
    terminated, time_out = bn > 1.0, ep > K.MAX_EPISODE_LENGTH
    reset = terminated | time_out
    pred["bn"], pred["terminated"], pred["time_out"] = bn, terminated, time_out
    # compute_reward :217-235, the 22 terms in alphabetical order
    s, _ = _sin_phase(ep, ct)
    stance = _stance(s)
    fzv = S["contact"][:, FEET, 2]
    contact = fzv > 5.0
    pred["s_rew"], pred["fz"], pred["contact"], pred["stance"] = s, fzv, contact, stance
    T = np.zeros((N, K.NUM_REWARDS))
    act, la, lla = S["actions"], S["last_actions"], S["last_last_actions"]
    T[:, 0] = np.sum((la - act) ** 2, 1) + np.sum((act + lla - 2 * la) ** 2, 1) + 0.05 * np.sum(np.abs(act), 1)      # :530-540
    T[:, 1] = np.exp(-np.sqrt(np.sum((S["last_root_vel"] - root[:, 7:13]) ** 2, 1)) * 3)                                # :386-393
    footz = S["rigid"][:, FEET, 2]
    mh = np.sum(footz * stance, 1) / np.sum(stance, 1)                                                                   # :374-384
    T[:, 2] = np.exp(-np.abs(root[:, 2] - (mh - F(0.05)) - F(K.BASE_HEIGHT_TARGET)) * 100)
    T[:, 3] = (bn > F(0.1)) * 1.0                                                                                        # :523-528
    jd = S["dof_pos"] - np.array(K.DEFAULT_DOF_POS)                                                                      # :362-372
    yr0 = np.sqrt(np.sum(jd[:, :2] ** 2, 1)) + np.sqrt(np.sum(jd[:, 6:8] ** 2, 1))
    T[:, 4] = np.exp(-np.clip(yr0 - F(0.1), 0, 50) * 100) - F(0.01) * np.sqrt(np.sum(jd ** 2, 1))
    pred["yr"] = yr0 - F(0.1)
    T[:, 5] = np.sum(((S["last_dof_vel"] - S["dof_vel"]) / dt) ** 2, 1)                                                  # :516-521
    T[:, 6] = np.sum(S["dof_vel"] ** 2, 1)                                                                               # :509-514
    fat0, lc = S["feet_air_time"], S["last_contacts"]                                                                    # :320-334
    filt = contact | (stance > 0.5) | lc
    first = (fat0 > 0.0) & filt
    air = fat0 + dt
    T[:, 7] = np.sum(np.clip(air, 0, 0.5) * first, 1)
    fat = air * ~filt
    pred["filt"], pred["first"], pred["air"], pred["fat0"], pred["lc"] = filt, first, air, fat0, lc
    z = footz - F(0.05)                                                                                                  # :446-467
    fh = S["feet_height"] + (z - S["last_feet_z"])
    near = np.abs(fh - F(K.TARGET_FEET_HEIGHT)) < F(0.01)
    T[:, 8] = np.sum(near * (1 - stance), 1)
    pred["near"], pred["fh_err"] = near, np.abs(fh - F(K.TARGET_FEET_HEIGHT))
    fh_new = fh * ~contact
    fn = np.sqrt(np.sum(S["contact"][:, FEET] ** 2, 2))                                                                  # :355-360
    T[:, 9] = np.sum(np.clip(fn - K.MAX_CONTACT_FORCE, 0, 400), 1)
    pred["fn_over"] = fn - K.MAX_CONTACT_FORCE
    T[:, 10] = np.mean(np.where(contact == (stance > 0.5), 1.0, F(-0.3)), 1)                                             # :336-344
    T[:, 11], pred["feet_d"] = _dist_term(S["rigid"][:, FEET, :2], K.MAX_DIST)
    T[:, 12] = np.sum(np.sqrt(np.sqrt(np.sum(S["rigid"][:, FEET, 7:9] ** 2, 2))) * contact, 1)                           # :308-318
    en = np.sqrt(np.sum((S["dof_pos"] - S["ref_dof_pos"]) ** 2, 1))                                                      # :272-280
    T[:, 13] = np.exp(-2 * en) - F(0.2) * np.clip(en, 0, 0.5)
    pred["joint_err"] = en
    T[:, 14], pred["knee_d"] = _dist_term(S["rigid"][:, KNEES, :2], K.MAX_DIST / 2)
    vx, cx = blv[:, 0], cmd[:, 0]                                                                                        # :469-500
    low, high = np.abs(vx) < 0.5 * np.abs(cx), np.abs(vx) > F(1.2) * np.abs(cx)
    ls = np.zeros(N)
    ls[low], ls[high], ls[~(low | high)] = -1.0, 0.0, F(1.2)
    ls[np.sign(vx) != np.sign(cx)] = -2.0
    live = np.abs(cx) > F(0.1)
    T[:, 15] = ls * live
    pred["ls"], pred["cx"], pred["live"] = ls, cx, live
    T[:, 16] = (np.exp(-np.sum(np.abs(eul[:, :2]), 1) * 10) + np.exp(-np.sqrt(np.sum(grav[:, :2] ** 2, 1)) * 20)) / 2.0  # :346-353
    T[:, 17] = np.sum(S["torques"] ** 2, 1)                                                                              # :502-507
    le2 = np.sum((cmd[:, :2] - blv[:, :2]) ** 2, 1)
    le, ae = np.sqrt(le2), np.abs(cmd[:, 2] - bav[:, 2])
    T[:, 18] = (np.exp(-le * 10) + np.exp(-ae * 10)) / 2.0 - F(0.2) * (le + ae)                                          # :408-425
    T[:, 19] = np.exp(-ae ** 2 * K.TRACKING_SIGMA)                                                                       # :436-444
    T[:, 20] = np.exp(-le2 * K.TRACKING_SIGMA)                                                                           # :427-434
    T[:, 21] = (np.exp(-blv[:, 2] ** 2 * 10) + np.exp(-np.sqrt(np.sum(bav[:, :2] ** 2, 1)) * 5.0)) / 2.0                 # :396-406
    scaled = T * np.array([F(v) for v in cfg["scales"]])
    total = np.zeros(N)
    for k in range(K.NUM_REWARDS):
        total = total + scaled[:, k]
    pred["sum_negative"] = total < 0
    rew = np.maximum(total, 0.0) if cfg["only_positive"] else total
    esum = S["episode_sums"] + scaled
    # reset_idx :163-215 + humanoid_env.py:264-269
    R = reset[:, None]
    dof_pos = np.where(R, np.array(K.DEFAULT_DOF_POS) + (F(0.2) * S["u_dof"] + F(-0.1)), S["dof_pos"])
    dof_vel = np.where(R, 0.0, S["dof_vel"])
    init = np.tile(np.array(K.BASE_INIT_STATE), (N, 1))
    init[:, :3] += S["env_origins"]
    root = np.where(R, init, root)
    cmd, _ = _resample(cmd, reset, S["u_cmd"][:, 3:6])
    zero = lambda a: np.where(R, 0.0, a)
    act, la, lla, ldv, fat = zero(act), zero(la), zero(lla), zero(S["last_dof_vel"]), zero(fat)
    ep = np.where(reset, 0, ep)
    cnt = max(int(reset.sum()), 1)
    extras = (esum * R).sum(0) / cnt / K.EPISODE_LENGTH_S
    esum = zero(esum)
    eul = np.where(R, _euler(root[:, 3:7])[0], eul)
    grav = np.where(R, _rot_inv(root[:, 3:7], np.tile([0.0, 0.0, -1.0], (N, 1))), grav)
    # compute_observations humanoid_env.py:200-262, newest frames
    s, co = _sin_phase(ep, ct)
    ref = _ref_pose(s)
    stance_o = _stance(s)
    pred["s_obs"] = s
    ci = np.stack((s, co, cmd[:, 0] * K.OBS_SCALE_LIN_VEL, cmd[:, 1] * K.OBS_SCALE_LIN_VEL, cmd[:, 2] * K.OBS_SCALE_ANG_VEL), 1)
    qq, dq = (dof_pos - np.array(K.DEFAULT_DOF_POS)) * K.OBS_SCALE_DOF_POS, dof_vel * F(K.OBS_SCALE_DOF_VEL)
    priv = np.concatenate((ci, qq, dq, act, dof_pos - ref, blv * K.OBS_SCALE_LIN_VEL, bav * K.OBS_SCALE_ANG_VEL, eul * K.OBS_SCALE_QUAT,
                           pf[:, :2], pt, S["friction"], S["body_mass"] / 30.0, stance_o, contact.astype(np.float64)), 1)
    frame = np.concatenate((ci, qq, dq, act, bav * K.OBS_SCALE_ANG_VEL, eul * K.OBS_SCALE_QUAT), 1)
    nv = np.zeros(K.NUM_SINGLE_OBS)
    nv[5:17], nv[17:29] = F(K.NOISE_DOF_POS * K.OBS_SCALE_DOF_POS), F(K.NOISE_DOF_VEL * K.OBS_SCALE_DOF_VEL)
    nv[41:44], nv[44:47] = F(K.NOISE_ANG_VEL * K.OBS_SCALE_ANG_VEL), F(K.NOISE_QUAT * K.OBS_SCALE_QUAT)
    frame = frame + S["z_obs"] * nv * F(K.NOISE_LEVEL)
    pred["obs_hi"], pred["obs_lo"] = (frame > K.CLIP_OBS).any(1), (frame < -K.CLIP_OBS).any(1)
    pred["priv_hi"], pred["priv_lo"] = (priv > K.CLIP_OBS).any(1), (priv < -K.CLIP_OBS).any(1)
    out = dict(reset=reset, time_out=time_out, episode_length=ep, rew=rew, terms=T, extras_episode=extras,
               commands=cmd, actions=act, last_actions=act, last_last_actions=la, last_dof_vel=dof_vel, last_root_vel=root[:, 7:13],
               feet_air_time=fat, feet_height=fh_new, last_feet_z=z, last_contacts=contact, ref_dof_pos=ref, push_force=pf, push_torque=pt,
               episode_sums=esum, base_lin_vel=blv, base_ang_vel=bav, projected_gravity=grav, base_euler=eul, root=root, dof_pos=dof_pos,
               dof_vel=dof_vel, frame=np.clip(frame, -K.CLIP_OBS, K.CLIP_OBS), priv=np.clip(priv, -K.CLIP_OBS, K.CLIP_OBS))
    return out, pred


# ------------------------------------------------------------------------------------------------ the case table
class Plan:
    """The pre-step state (P), the step's inputs and the sim frame of N envs, as fp32 torch tensors a case may overwrite row by row."""

    def __init__(self, N, g, cycle_time):
        self.N = N
        r, rn = (lambda *s: torch.rand(*s, generator=g)), (lambda *s: torch.randn(*s, generator=g))
        self.ep_len = torch.randint(70, 700, (N,), generator=g)
        self.commands = None                      # from the primed oracle
        P = self.P = {}
        P["actions"], P["last_actions"], P["last_last_actions"] = rn(N, 12) * 0.5, rn(N, 12) * 0.5, rn(N, 12) * 0.5
        P["last_dof_vel"], P["last_root_vel"] = rn(N, 12) * 1.5, rn(N, 6) * 0.3
        P["feet_air_time"] = r(N, 2) * 0.3 * (r(N, 2) > 0.5)
        P["feet_height"], P["last_feet_z"] = r(N, 2) * 0.05, r(N, 2) * 0.05
        P["push_force"], P["push_torque"] = rn(N, 3) * 0.1, rn(N, 3) * 0.1
        P["push_force"][:, 2] = 0.0
        P["episode_sums"] = torch.zeros(N, K.NUM_REWARDS)
        self.last_contacts = r(N, 2) > 0.5
        self.pre_dof_pos, self.pre_dof_vel = rn(N, 12) * 0.2, rn(N, 12) * 1.5
        self.a_in, self.u_delay, self.z_act = rn(N, 12) * 1.5, r(N), rn(N, 12)
        self.frame = EC.synth_frames(g, N)
        self.root, self.dof = self.frame[0], self.frame[1].view(N, 12, 2)
        self.contact, self.rigid = self.frame[2].view(N, K.NUM_BODIES, 3), self.frame[3].view(N, K.NUM_BODIES, 13)
        # feet_contact_forces = |F| - 700 clipped: for |F| in (700, 706.1) one ulp of |F| (6.1e-5) is more than 1e-5 of the term, so
        # two correct fp32 evaluations of the norm that differ in the last bit miss the per-term bar (measured on an ordinary env at
        # scale 1: 1.6e-5 relative, 6.1e-5 absolute).  Ordinary envs are moved out of that strip; the threshold itself is
        # covered by planted cases whose norms are exact in fp32: (0, 0, 706.25), the first point from which one ulp of |F| is within the bar
        # (the device's square root is the 1-ulp hardware one), and (0, 0, 1100).
        fn = self.contact[:, FEET].norm(dim=-1)
        self.contact[:, FEET, 2] += 10.0 * ((fn > K.MAX_CONTACT_FORCE - 1.0) & (fn < K.MAX_CONTACT_FORCE + 8.0))
        self.u_cmd, self.u_dof, self.u_push, self.z_obs = r(N, 6), r(N, 12), r(N, 5), rn(N, 47)
        self.cycle_time = cycle_time
        self.keep_fast = []                       # rows whose joint / base velocities stay beyond the observation clip in the later steps
        self.joint_err = []                       # (row, norm): joint angles to be set that far from the stored reference pose (finish)
        self.rows = []                            # the case rows, in CASES order (build)
        self.ref_dof_pos = None

    def finish(self, commands):
        """Apply the cases.  Called once, with the primed commands of the ordinary rows (cases overwrite their own): every case row is
        made quiet first, then planted; the stored reference pose follows the planted episode lengths, and the joint_pos cases are
        placed relative to it."""
        self.commands = commands.clone()
        for i in self.rows:
            self.quiet(i)
        for (name, edge, fn), i in zip(CASES, self.rows):
            fn(self, i)
        self.ref_dof_pos = self.ref_pose()
        for i, v in self.joint_err:
            self.dof[i, :, 0] = self.ref_dof_pos[i]
            self.dof[i, 2, 0] += v

    def quiet(self, i):
        """A case row starts ordinary but with nothing else going on: no base contact, identity attitude, off every gait / resample edge."""
        self.contact[i, BASE] = 0.0
        self.ep_len[i] = 73                         # -> 74: sin(phase) = 0.83 at cycle_time 0.64, 0.996 at CYCLE_EXACT: left foot stance
        self.root[i, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])

    def ref_pose(self):
        """ref_dof_pos as the previous compute_observations left it (humanoid_env.py:121-142) for the planted episode lengths."""
        s, _ = _sin_phase(self.ep_len.numpy(), self.cycle_time)
        return torch.from_numpy(_ref_pose(np.float32(s).astype(np.float64))).float()


CASES = []


def case(name, edge, fn):
    CASES.append((name, edge, fn))


def _feet(attr, comp, vals):
    def fn(p, i):
        for f, v in enumerate(vals):
            getattr(p, attr)[i, FEET[f], comp] = v
    return fn


def _chain(*fns):
    def fn(p, i):
        for f in fns:
            f(p, i)
    return fn


def _set(attr, idx, val, P=False):
    def fn(p, i):
        t = p.P[attr] if P else getattr(p, attr)
        if idx is None:
            t[i] = torch.as_tensor(val, dtype=t.dtype)
        else:
            t[i, idx] = torch.as_tensor(val, dtype=t.dtype)
    return fn


def _build_cases():
    # ---- contact: fz on 5.0 and its two neighbours (contact is `fz > 5`)
    for nm, v in (("at", 5.0), ("above", up(5.0)), ("below", dn(5.0))):
        case("contact fz " + nm, "contact", _chain(_feet("contact", 2, (v, v)), _set("feet_air_time", None, [0.2, 0.2], P=True)))
    # ---- feet_air_time: last_contacts x contact (the left foot is in stance, the right one swings), then the clamp of `air`
    for lc in (0, 1):
        for con in (0.0, 300.0):
            case("air filt lc=%d contact=%d" % (lc, con > 0), "air_time",
                 _chain(_feet("contact", 2, (con, con)), _set("last_contacts", None, [bool(lc)] * 2), _set("feet_air_time", None, [0.2, 0.2], P=True)))
    for nm, v in (("zero", 0.0), ("just over zero", 1e-6), ("lands on 0.5", 0.49), ("beyond 0.5", 0.7)):
        case("air " + nm, "air_time", _chain(_feet("contact", 2, (300.0, 300.0)), _set("feet_air_time", None, [v, v], P=True)))
    case("contact number L only", "contact_number", _feet("contact", 2, (300.0, 0.0)))
    case("contact number R only", "contact_number", _feet("contact", 2, (0.0, 300.0)))
    # ---- base contact: exactly representable norms around collision (> 0.1) and termination (> 1.0)
    for nm, v in (("(1,0,0)", [1.0, 0, 0]), ("(1+,0,0)", [up(1.0), 0, 0]), ("(1-,0,0)", [dn(1.0), 0, 0]), ("(0,0,0.1f)", [0, 0, F(0.1)]),
                  ("(0,0,0.1f+)", [0, 0, up(0.1)]), ("(0,0,0.1f-)", [0, 0, dn(0.1)]), ("(0,0,0)", [0, 0, 0])):
        case("base contact " + nm, "base_contact", _set("contact", BASE, v))
    M = K.MAX_EPISODE_LENGTH
    for ep in (M - 2, M - 1, M):
        case("episode length %d" % ep, "time_out", _set("ep_len", None, ep))
    case("terminated and timed out", "time_out", _chain(_set("ep_len", None, M), _set("contact", BASE, [0.0, 3.0, 0.0])))
    case("terminated one step before the time-out", "time_out", _chain(_set("ep_len", None, M - 1), _set("contact", BASE, [0.0, 0.0, -2.0])))
    # ---- feet_contact_forces: clip(|F| - 700, 0, 400)
    for nm, v in (("below max", [0, 0, 650.0]), ("just above max", [0, 0, 706.25]), ("+350", [0, 0, 1050.0]), ("at +400", [0, 0, 1100.0]),
                  ("well beyond +400", [300.0, 400.0, 5000.0])):
        case("feet force " + nm, "feet_forces", lambda p, i, v=v: [p.contact[i, FEET[0]].copy_(torch.tensor(v)), p.contact[i, FEET[1]].copy_(torch.tensor(v))])
    # ---- feet_clearance: |feet_height - 0.06| against 0.01, swing (right) and stance (left) foot; feet_height zeroed on contact
    for nm, d, con in (("near, no contact", 0.009, 0.0), ("far, no contact", 0.011, 0.0), ("near, contact", -0.009, 300.0), ("far, contact", -0.011, 300.0)):
        def fn(p, i, d=d, con=con):
            p.P["last_feet_z"][i] = p.rigid[i, FEET, 2] - 0.05          # this step's delta_z is exactly zero
            p.P["feet_height"][i] = K.TARGET_FEET_HEIGHT + d
            p.contact[i, FEET[0], 2], p.contact[i, FEET[1], 2] = con, con
        case("clearance " + nm, "clearance", fn)
    # ---- feet / knee distance: below min_dist, inside the band, above max, above max + 0.5.  (The lower clamp -0.5 of d_min cannot
    # bind, d >= 0 > min_dist - 0.5: nothing is planted for it.)
    for who, bodies, ds in (("feet", FEET, (0.1, 0.35, 0.7, 1.2)), ("knee", KNEES, (0.1, 0.22, 0.4, 0.9))):
        for d in ds:
            def fn(p, i, bodies=bodies, d=d):
                p.rigid[i, bodies[0], 0:2] = torch.tensor([0.02, d / 2])
                p.rigid[i, bodies[1], 0:2] = torch.tensor([0.02, -d / 2])
            case("%s distance %.2f" % (who, d), who + "_distance", fn)
    # ---- joints
    for nm, v in (("below 0.1", 0.03), ("above 0.1", 0.3), ("above 50.1", 60.0)):
        def fn(p, i, v=v):
            p.dof[i, :, 0] = 0.0
            p.dof[i, 0, 0] = v
        case("yaw-roll deviation " + nm, "yaw_roll", fn)
    for nm, v in (("below 0.5", 0.3), ("above 0.5", 0.8)):
        case("joint_pos error " + nm, "joint_pos", lambda p, i, v=v: p.joint_err.append((i, v)))
    for nm, qv in (("above +limit", -1.0), ("below -limit", 1.0)):
        case("torque " + nm, "torques", _set("pre_dof_pos", None, [qv] * 12))
    for sgn in (1.0, -1.0):
        for nm, u in (("no delay", 0.0), ("delay close to 1", float(np.nextafter(np.float32(1.0), np.float32(0.0))))):
            case("action %+d x clip, %s" % (sgn * 40, nm), "actions",
                 _chain(_set("a_in", None, [sgn * 40.0] * 12), _set("u_delay", None, u), _set("z_act", None, [2.0, -2.0] * 6)))
    # ---- gait phase (episode length BEFORE the step; the step adds one): sin in the double-stance band, just outside it on either sign
    for ep in (0, 1, 4, 30, 31, 32, 33, 62, 63):
        case("gait episode length %d" % ep, "gait", _set("ep_len", None, ep))
    # ---- commands
    for nm, v in (("0.1f", F(0.1)), ("0.1f+", up(0.1)), ("0.1f-", dn(0.1)), ("-0.1f", -F(0.1)), ("-0.1f-", -up(0.1))):
        case("cx " + nm, "cx", _chain(_set("commands", 0, v), _set("root", slice(7, 10), [0.09 * np.sign(v), 0.0, 0.0])))
    for nm, ep, u0 in (("norm 0.15", 799, 0.5), ("norm 0.24", 799, 0.6), ("norm 0.51", 1599, 0.9), ("one step early", 798, 0.5)):
        case("resample " + nm, "resample", _chain(_set("ep_len", None, ep), _set("u_cmd", slice(0, 3), [u0, 0.5, 0.5]), _set("commands", None, [0.3, 0.1, 0.0, 0.4])))
    for nm, h in (("+3.0", 3.0), ("-3.0", -3.0), ("0", 0.0), ("just below 0", -1e-7), ("+3.5", 3.5), ("-3.5", -3.5), ("0.8", 0.8)):
        case("heading target " + nm, "heading", _set("commands", 3, h))
    for nm, vx, cx in (("low", 0.1, 0.5), ("high", 0.9, 0.5), ("desired", 0.5, 0.5), ("sign mismatch", -0.5, 0.5), ("dead band", 0.04, 0.05)):
        case("low_speed " + nm, "low_speed", _chain(_set("commands", 0, cx), _set("root", slice(7, 10), [vx, 0.0, 0.0])))
    # ---- orientation
    h = 0.70710684
    for nm, qv in (("gimbal +", [0, h, 0, h]), ("gimbal -", [0, -h, 0, h]), ("large roll", [math.sin(1.2), 0, 0, math.cos(1.2)]), ("identity", [0, 0, 0, 1.0]),
                   ("scaled by 1e-12", [0.1e-12, 0.05e-12, 0.02e-12, 1e-12]), ("zero", [0, 0, 0, 0])):
        case("quaternion " + nm, "orientation", _set("root", slice(3, 7), qv))
    # ---- observation clip: elements of the newest frames beyond +-18, kept there in the later steps so that clipped frames fill the ring
    def fast(sgn, what):
        def fn(p, i):
            if what == "joints":
                p.dof[i, :, 1] = torch.tensor([400.0, -400.0] * 6) * sgn
            elif what == "base":
                p.root[i, 7:13] = torch.tensor([12.0, -12.0, 12.0, 25.0, -25.0, 25.0]) * sgn
            else:
                p.z_obs[i] = torch.tensor([3000.0, -3000.0] * 23 + [3000.0]) * sgn
            p.keep_fast.append((i, sgn, what))
        return fn
    for what in ("joints", "base", "noise"):
        for sgn in (1.0, -1.0):
            case("observation clip %s %+d" % (what, sgn), "obs_clip", fast(sgn, what))
    # ---- push draws at the ends of their range (the pass decides whether the step pushes)
    case("push uniforms 0", "push", _set("u_push", None, [0.0] * 5))
    case("push uniforms close to 1", "push", _set("u_push", None, [float(np.nextafter(np.float32(1.0), np.float32(0.0)))] * 5))
    # ---- reward sum: an ordinary walking env (positive scaled sum) and one whose penalties win
    case("reward sum positive", "reward_sum", lambda p, i: None)
    case("reward sum negative", "reward_sum", _chain(_set("contact", BASE, [0.0, 0.0, 0.5]), lambda p, i: p.dof[i, :, 1].fill_(30.0)))


_build_cases()
assert len(CASES) == NUM_CASES, len(CASES)


def census(built):
    """{edge: {side: count}} over the case rows of every pass, from the float64 reference's predicates."""
    C = {}

    def add(edge, side, mask):
        C.setdefault(edge, {}).setdefault(side, 0)
        C[edge][side] += int(np.sum(mask))
    for pname, b in built.items():
        rows, p, pre = b["rows"], {k: v[b["rows"]] for k, v in b["R"][1].items()}, {k: v[b["rows"]] for k, v in b["pre_pred"].items()}
        o = {k: v[rows] for k, v in b["R"][0].items() if isinstance(v, np.ndarray) and v.shape[:1] == (b["N"],)}
        fz = p["fz"]
        add("contact fz", "on 5.0", fz == 5.0); add("contact fz", "next above", fz == up(5.0)); add("contact fz", "next below", fz == dn(5.0))
        for lc in (0, 1):
            for con in (0, 1):
                add("air_time last_contacts x contact", "lc=%d contact=%d" % (lc, con), (p["lc"] == bool(lc)) & (p["contact"] == bool(con)))
        add("air_time filt", "true", p["filt"]); add("air_time filt", "false", ~p["filt"])
        add("air_time first", "true", p["first"]); add("air_time first", "false", ~p["first"])
        add("air clamp", "air_time 0", p["fat0"] == 0); add("air clamp", "inside", p["first"] & (p["air"] < 0.499))
        add("air clamp", "lands on 0.5", p["first"] & (np.abs(p["air"] - 0.5) < 1e-6)); add("air clamp", "beyond 0.5", p["first"] & (p["air"] > 0.51))
        eq = p["contact"] == (p["stance"] > 0.5)
        for f, nm in enumerate(("left", "right")):
            add("contact number " + nm, "contact == stance", eq[:, f]); add("contact number " + nm, "contact != stance", ~eq[:, f])
        bn = p["bn"]
        for thr, nm in ((1.0, "termination"), (F(0.1), "collision")):
            add(nm + " norm", "on threshold", bn == thr); add(nm + " norm", "next above", bn == up(thr)); add(nm + " norm", "next below", bn == dn(thr))
        add("collision norm", "zero", bn == 0)
        for t in (0, 1):
            for to in (0, 1):
                add("termination x time-out", "terminated=%d timed_out=%d" % (t, to), (p["terminated"] == bool(t)) & (p["time_out"] == bool(to)))
        fo = p["fn_over"]
        add("feet forces", "below max", fo < 0); add("feet forces", "inside the clamp", (fo > 0) & (fo < 400))
        add("feet forces", "between +300 and +400", (fo > 300) & (fo < 400)); add("feet forces", "on +400", fo == 400); add("feet forces", "beyond +400", fo > 400)
        swing = p["stance"] < 0.5
        for nm, m in (("swing", swing), ("stance", ~swing)):
            add("clearance " + nm, "near", p["near"] & m); add("clearance " + nm, "far", ~p["near"] & m)
        add("feet_height on contact", "zeroed", p["contact"]); add("feet_height on contact", "kept", ~p["contact"])
        for who, mx in (("feet", K.MAX_DIST), ("knee", K.MAX_DIST / 2)):
            d = p[who + "_d"]
            add(who + " distance", "below min", d < K.MIN_DIST); add(who + " distance", "in the band", (d > K.MIN_DIST) & (d < mx))
            add(who + " distance", "above max", (d > mx) & (d < mx + 0.5)); add(who + " distance", "above max + 0.5", d > mx + 0.5)
        add("yaw-roll", "below 0.1", p["yr"] < 0); add("yaw-roll", "inside", (p["yr"] > 0) & (p["yr"] < 50)); add("yaw-roll", "above 50.1", p["yr"] > 50)
        add("joint_pos error", "below 0.5", p["joint_err"] < 0.5); add("joint_pos error", "above 0.5", p["joint_err"] > 0.5)
        add("torque limit", "above +limit", pre["tq_hi"]); add("torque limit", "below -limit", pre["tq_lo"]); add("torque limit", "inside", pre["tq_in"])
        add("action clip", "above +clip", pre["a_hi"]); add("action clip", "below -clip", pre["a_lo"]); add("action clip", "second clip binds", pre["a2_clip"])
        add("action delay", "u = 0", b["S"]["u_delay"][rows] == 0); add("action delay", "u close to 1", b["S"]["u_delay"][rows] > 0.9999)
        s = p["s_rew"]
        add("gait sin", "double stance", np.abs(s) < F(0.1)); add("gait sin", "just outside +", (s > F(0.1)) & (s < 0.2))
        add("gait sin", "just outside -", (s < -F(0.1)) & (s > -0.2)); add("gait sin", "exactly 0 (observation after a reset)", p["s_obs"] == 0)
        add("gait sin", "within 1 ulp of 0.1f, not below it", (s >= F(0.1)) & (s - F(0.1) < float(np.spacing(np.float32(0.1)))))
        acx = np.abs(p["cx"])
        add("|cx|", "on 0.1f", acx == F(0.1)); add("|cx|", "next above", acx == up(0.1)); add("|cx|", "next below", acx == dn(0.1))
        add("resample", "on the step, norm above 0.2", p["resample"] & (p["cmd_norm"] > 0.2)); add("resample", "norm between 0.2 and 0.25", p["resample"] & (p["cmd_norm"] > 0.2) & (p["cmd_norm"] < 0.25))
        add("resample", "on the step, norm below 0.2", p["resample"] & (p["cmd_norm"] < 0.2)); add("resample", "one step early", b["S"]["ep_len"][rows] == 798)
        add("heading clamp", "+1 binds", p["half_ang"] > 1); add("heading clamp", "-1 binds", p["half_ang"] < -1); add("heading clamp", "inside", np.abs(p["half_ang"]) < 1)
        hd = p["heading_diff"]
        add("heading wrap", "0", hd == 0); add("heading wrap", "just below 0", (hd < 0) & (hd > -1e-6)); add("heading wrap", "beyond +pi", hd > math.pi); add("heading wrap", "beyond -pi", hd < -math.pi)
        for nm, v in (("too low", -1.0), ("too high", 0.0), ("desired", F(1.2)), ("sign mismatch", -2.0)):
            add("low_speed", nm, p["live"] & (p["ls"] == v))
        add("low_speed", "dead band", ~p["live"])
        add("euler pitch", "gimbal +", p["sp"] >= 1); add("euler pitch", "gimbal -", p["sp"] <= -1); add("euler pitch", "asin", np.abs(p["sp"]) < 1)
        add("euler roll", "large", np.abs(o["base_euler"][:, 0]) > 1); add("quaternion norm", "below 1e-9", np.sqrt((b["S"]["root"][rows, 3:7] ** 2).sum(1)) < 1e-9)
        add("observation clip", "obs above +18", p["obs_hi"]); add("observation clip", "obs below -18", p["obs_lo"])
        add("observation clip", "priv above +18", p["priv_hi"]); add("observation clip", "priv below -18", p["priv_lo"])
        add("push", "on the interval", p["pushed"]); add("push", "one step before", ~p["pushed"])
        add("push uniforms", "0", (b["S"]["u_push"][rows] == 0).all(1)); add("push uniforms", "close to 1", (b["S"]["u_push"][rows] > 0.9999).all(1))
        add("reward sum", "negative, clipped", p["sum_negative"] & b["cfg"]["only_positive"]); add("reward sum", "negative, kept", p["sum_negative"] & (not b["cfg"]["only_positive"]))
        add("reward sum", "positive", ~p["sum_negative"])
    return C


# ------------------------------------------------------------------------------------------------ builder
def make_pair(plan, cfg, backend=None, sim_layout="soa", rows_ahead=False):
    """A primed oracle (and, with a backend, the product env) holding the plan's pre-step state."""
    N = plan.N
    g = torch.Generator().manual_seed(9000 + N)
    fr, bm = 0.1 + 1.9 * torch.rand(N, 1, generator=g), 10.0 + 10.0 * torch.rand(N, 1, generator=g)
    o = XBotEnvOracle(N, frictions=fr, body_mass=bm, reward_scales_dt=cfg["scales"], only_positive_rewards=cfg["only_positive"],
                      cycle_time=cfg["cycle_time"])
    draws = torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g), torch.randn(N, 47, generator=g)
    o.prime(*draws)
    env = None
    if backend is not None:
        env = EC.EnvUnderTest(backend, N, fr, bm, sim_layout=sim_layout, rows_ahead=rows_ahead)
        for k in range(K.NUM_REWARDS):
            env.cfg.reward_scales[k] = cfg["scales"][k]
        env.cfg.only_positive_rewards = int(cfg["only_positive"])
        env.cfg.cycle_time = cfg["cycle_time"]
        env.prime(*draws)
        backend.sync()
    if plan.commands is None:              # the primed commands are the ordinary rows' commands
        plan.finish(o.commands)
    o.ep_len = plan.ep_len.clone()
    o.commands = plan.commands.clone()
    for name, t in plan.P.items():
        setattr(o, name, t.clone())
    o.ref_dof_pos = plan.ref_dof_pos.clone()
    o.last_contacts = plan.last_contacts.clone()
    o.sim.dof_pos.copy_(plan.pre_dof_pos)
    o.sim.dof_vel.copy_(plan.pre_dof_vel)
    o.common_step_counter = cfg["csc"]
    if env is not None:
        b = env.buf
        b.episode_length.copy_(plan.ep_len)
        b.view("commands").copy_(plan.commands)
        for name, t in plan.P.items():
            b.view(name).copy_(t)
        b.view("ref_dof_pos").copy_(plan.ref_dof_pos)
        b.view("last_contacts").copy_(plan.last_contacts.float())
        b.dof_pos_view().copy_(plan.pre_dof_pos)
        b.dof_vel_view().copy_(plan.pre_dof_vel)
        b.counters[L.CNT_STEP] = cfg["csc"]
    return o, env


def oracle_step(o, plan):
    a = plan.a_in.clone()
    o.pre_physics(a, plan.u_delay, plan.z_act)
    o.pd_torques()
    o.sim.load(*plan.frame)
    return o.post_physics(plan.u_cmd, plan.u_dof, plan.u_push, plan.z_obs)


_BUILT = {}
FIELDS64 = ("commands", "actions", "last_actions", "last_last_actions", "last_dof_vel", "last_root_vel", "feet_air_time", "feet_height",
            "last_feet_z", "ref_dof_pos", "push_force", "push_torque", "base_lin_vel", "base_ang_vel", "projected_gravity", "base_euler")


def bar(name, ref):
    """The project's fp32 bar around a reference value (env_common.RTOL / ATOL, the torque floor of compare_state)."""
    return (2e-5 if name == "torques" else EC.ATOL) + EC.RTOL * np.abs(ref)


def product_views(o):
    """name -> array, for the oracle object (the product side goes through env_views)."""
    n = lambda t: t.detach().cpu().double().numpy()
    v = {k: n(getattr(o, k)) for k in FIELDS64}
    v.update(torques=n(o.torques), rew=n(o.rew), root=n(o.sim.root), dof_pos=n(o.sim.dof_pos), dof_vel=n(o.sim.dof_vel),
             frame=n(torch.clip(o.obs[:, -K.NUM_SINGLE_OBS:], -K.CLIP_OBS, K.CLIP_OBS)),
             priv=n(torch.clip(o.priv[:, -K.SINGLE_NUM_PRIV_OBS:], -K.CLIP_OBS, K.CLIP_OBS)), episode_sums=n(o.episode_sums),
             extras_episode=n(o.extras_episode))
    return v


def env_views(env):
    b = env.buf
    n = lambda t: t.detach().cpu().double().numpy()
    v = {k: n(b.view(k)) for k in FIELDS64}
    v.update(torques=n(b.view("torques")), rew=n(b.rew), root=n(b.root_view()), dof_pos=n(b.dof_pos_view()), dof_vel=n(b.dof_vel_view()),
             frame=n(b.obs[:, -K.NUM_SINGLE_OBS:]), priv=n(b.priv_obs[:, -K.SINGLE_NUM_PRIV_OBS:]), episode_sums=n(b.view("episode_sums")),
             extras_episode=n(b.extras_episode))
    return v


def distances(views, b):
    """Largest distance from the float64 reference, in units of the fp32 bar: {field or "term <name>": value}.  The terms are read
    from the episode sums of the envs that did not reset (they were zero before the step)."""
    R, act64, tq64 = b["R"][0], b["act64"], b["tq64"]
    D = {}
    for k in FIELDS64 + ("rew", "root", "dof_pos", "dof_vel", "frame", "priv"):
        D[k] = float(np.max(np.abs(views[k] - R[k]) / bar(k, R[k])))
    D["actions (filter)"] = float(np.max(np.abs(np.where(R["reset"][:, None], 0.0, views["actions"] - act64)) / bar("actions", act64)))
    D["torques"] = float(np.max(np.abs(views["torques"] - tq64) / bar("torques", tq64)))
    live = ~R["reset"]
    for k, name in enumerate(K.REWARD_NAMES):
        ref = R["episode_sums"][live, k]
        D["term " + name] = float(np.max(np.abs(views["episode_sums"][live, k] - ref) / bar("term", ref)))
    D["extras_episode"] = float(np.max(np.abs(views["extras_episode"] - R["extras_episode"]) / (1e-7 + 1e-5 * np.abs(R["extras_episode"]))))
    return D


def build(pass_name, nfill=55):
    """The planted table of one pass with `nfill` ordinary envs around the cases: the plan, both references' results, the fp32
    oracle's distance from the float64 reference, and the side-agreement check.  Cached."""
    key = (pass_name, nfill)
    if key in _BUILT:
        return _BUILT[key]
    cfg = PASSES[pass_name]
    N = NUM_CASES + nfill
    g = torch.Generator().manual_seed(4196 + nfill)
    plan = Plan(N, g, cfg["cycle_time"])
    rows = torch.randperm(N, generator=g)[:NUM_CASES]

    plan.rows = rows.tolist()
    o, _ = make_pair(plan, cfg)
    w = lambda t: t.detach().double().numpy().copy()
    S = {k: w(v) for k, v in plan.P.items()}
    S.update(ep_len=plan.ep_len.numpy().copy(), commands=w(plan.commands), ref_dof_pos=w(plan.ref_dof_pos), last_contacts=plan.last_contacts.numpy().copy(),
             pre_dof_pos=w(plan.pre_dof_pos), pre_dof_vel=w(plan.pre_dof_vel), root=w(plan.root), dof_pos=w(plan.dof[:, :, 0]), dof_vel=w(plan.dof[:, :, 1]),
             contact=w(plan.contact), rigid=w(plan.rigid), u_cmd=w(plan.u_cmd), u_dof=w(plan.u_dof), u_push=w(plan.u_push), z_obs=w(plan.z_obs),
             u_delay=w(plan.u_delay), friction=w(o.friction), body_mass=w(o.body_mass), env_origins=w(o.env_origins))
    act64, tq64, pre_pred = ref64_pre(S, w(plan.a_in), w(plan.u_delay), w(plan.z_act))
    oracle_step(o, plan)
    # the post-physics step takes the fp32 oracle's filtered actions and torques, widened: every fp32 input exact
    S["actions"], S["torques"] = w(_pre_reset_actions(plan)), w(o.torques)
    R = ref64_step(S, cfg)
    b = dict(plan=plan, cfg=cfg, N=N, rows=rows.numpy(), S=S, R=R, act64=act64, tq64=tq64, pre_pred=pre_pred, oracle=o)
    # the two references take the same side of every predicate: masks and integer state exact, and every step-function output equal
    out = R[0]
    assert np.array_equal(out["reset"], o.reset.numpy()) and np.array_equal(out["time_out"], o.time_out.numpy()), "badly built case: termination"
    assert np.array_equal(out["episode_length"], o.ep_len.numpy()) and np.array_equal(out["last_contacts"], o.last_contacts.numpy())
    names = {i: n for (n, _, _), i in zip(CASES, plan.rows)}
    who = lambda mask: [names.get(int(i), "ordinary env %d" % i) for i in np.nonzero(mask)[0]]
    scales = np.array([F(v) for v in cfg["scales"]])
    ot = o.reward_terms.double().numpy()
    for k in ("collision", "feet_air_time", "feet_clearance", "feet_contact_number", "low_speed"):     # the step-function terms, row by row
        j = K.REWARD_NAMES.index(k)
        flip = np.abs(ot[:, j] - out["terms"][:, j] * scales[j]) > 1e-3 * abs(scales[j])
        assert not flip.any(), "badly built case: the references take different sides in %s: %r" % (k, who(flip))
    live = ~out["reset"]
    opriv = o.priv[:, -K.SINGLE_NUM_PRIV_OBS:].double().numpy()
    flip = (np.abs(opriv[:, 69:73] - out["priv"][:, 69:73]) > 0.5).any(1)
    assert not flip.any(), "badly built case: stance / contact entries differ: %r" % who(flip)
    flip = ((o.commands[:, :2].numpy() == 0) != (out["commands"][:, :2] == 0)).any(1)
    assert not flip.any(), "badly built case: the 0.2 command dead band: %r" % who(flip)
    flip = (np.abs(o.ref_dof_pos.double().numpy() - out["ref_dof_pos"]) > 1e-3).any(1)
    assert not flip.any(), "badly built case: the double-stance band of the reference pose: %r" % who(flip)
    views = product_views(o)
    D = b["oracle_distance"] = distances(views, b)
    # measured: 2.74 bars at most (the gait clock's fp32 argument late in an episode); anything beyond 4 is a drifted case or an oracle defect
    worst = {k: v for k, v in D.items() if v > 4.0}
    assert not worst, "the fp32 oracle is further from the float64 reference than ever measured: %r" % worst
    assert np.all(np.isfinite(views["frame"])) and np.all(np.isfinite(out["frame"])) and np.all(np.isfinite(out["rew"])) and np.all(np.isfinite(views["rew"]))
    _BUILT[key] = b
    return b


def _pre_reset_actions(plan):
    """The fp32 oracle's filtered actions of this step (post_physics zeroes them for the envs it resets: redo the filter)."""
    o2 = XBotEnvOracle(plan.N)
    o2.actions = plan.P["actions"].clone()
    return o2.pre_physics(plan.a_in.clone(), plan.u_delay, plan.z_act)


def build_all(nfill=55):
    built = {p: build(p, nfill) for p in PASSES}
    C = census(built)
    empty = [(e, s) for e, sides in C.items() for s, n in sides.items() if n == 0]
    assert not empty, "census: no case on %r" % empty
    return built, C


def allowance(D_oracle, key):
    return max(1.0, 4.0 * D_oracle[key])


# ------------------------------------------------------------------------------------------------ runner
ERRORS = {}        # (backend name, pass) -> {key: (oracle distance, product's largest error)} in units of the fp32 bar, for the report


def run_table(backend, pass_name, sim_layout="soa", rows_ahead=False, nfill=55, more_steps=0):
    """The planted step of one pass through `backend`, against both references; then `more_steps` ordinary steps against the fp32
    oracle, in which the rows of the observation-clip cases stay beyond the clip so that clipped frames reach every ring slot."""
    b = build(pass_name, nfill)
    plan, cfg = b["plan"], b["cfg"]
    o, env = make_pair(plan, cfg, backend, sim_layout, rows_ahead)
    oracle_step(o, plan)
    env.step(plan.a_in, plan.frame, plan.u_delay, plan.z_act, plan.u_cmd, plan.u_dof, plan.u_push, plan.z_obs)
    tag = "%s pass, planted step" % pass_name
    EC.compare_state(env, o, tag)                        # fp32 oracle, per term (episode_sums), masks exact
    R = b["R"][0]
    EC.exact(env.buf.reset, R["reset"], tag + " reset vs float64")
    EC.exact(env.buf.time_out, R["time_out"], tag + " time_out vs float64")
    EC.exact(env.buf.episode_length, R["episode_length"], tag + " episode_length vs float64")
    EC.exact(env.buf.view("last_contacts") > 0.5, R["last_contacts"], tag + " last_contacts vs float64")
    D = distances(env_views(env), b)
    rec = ERRORS.setdefault((backend.name, pass_name), {})
    bad = {}
    for k, v in D.items():
        rec[k] = (b["oracle_distance"][k], max(v, rec.get(k, (0, 0))[1]))
        if v > allowance(b["oracle_distance"], k):
            bad[k] = (v, allowance(b["oracle_distance"], k))
    assert not bad, "%s: beyond max(fp32 bar, 4 x oracle distance) from the float64 reference (error, allowance; units of the bar): %r" % (tag, bad)
    g = torch.Generator().manual_seed(77)
    N = plan.N
    for t in range(more_steps):
        a_in = torch.randn(N, 12, generator=g) * 1.5
        frame = EC.synth_frames(g, N)
        z_obs = torch.randn(N, 47, generator=g)
        for i, sgn, what in plan.keep_fast:
            frame[0][i, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
            frame[2].view(N, K.NUM_BODIES, 3)[i, BASE] = 0.0
            if what == "joints":
                frame[1].view(N, 12, 2)[i, :, 1] = torch.tensor([400.0, -400.0] * 6) * sgn
            elif what == "base":
                frame[0][i, 7:13] = torch.tensor([12.0, -12.0, 12.0, 25.0, -25.0, 25.0]) * sgn
            else:
                z_obs[i] = torch.tensor([3000.0, -3000.0] * 23 + [3000.0]) * sgn
        nz = [torch.rand(N, generator=g), torch.randn(N, 12, generator=g), torch.rand(N, 6, generator=g), torch.rand(N, 12, generator=g),
              torch.rand(N, 5, generator=g), z_obs]
        a_o = a_in.clone()
        o.pre_physics(a_o, nz[0], nz[1]); o.pd_torques(); o.sim.load(*frame); o.post_physics(*nz[2:])
        env.step(a_in, frame, *nz)
        EC.compare_state(env, o, "%s pass, later step %d" % (pass_name, t))
    if more_steps:
        rows = [i for i, _, _ in plan.keep_fast]
        H = K.FRAME_STACK
        stacked = env.buf.obs.detach().cpu()[rows].view(len(rows), H, K.NUM_SINGLE_OBS)
        on_clip = (stacked.abs() == K.CLIP_OBS).flatten(2).any(2)
        assert more_steps < H - 1 or bool(on_clip.all()), "a clipped frame did not reach every slot of the stacked row"
    return env, o


def report_errors(backend_name, pass_name):
    """The float64 error table of one run into the terminal summary (synth_common.REPORT), pass or fail, and to stdout."""
    import synth_common as SC
    rec = ERRORS.get((backend_name, pass_name), {})
    worst = sorted(rec.items(), key=lambda kv: -kv[1][1])[:8]
    line = "edge suite, %s backend, %s pass, float64 distances in fp32 bars (oracle / product), largest: %s" % (
        backend_name, pass_name, "; ".join("%s %.3f / %.3f" % (k, a, c) for k, (a, c) in worst))
    SC.REPORT.append((line, 0))
    print(error_table())


def error_table():
    """The report: per pass and backend, the fp32 oracle's distance from the float64 reference and the product's largest error,
    both in units of the fp32 bar (ATOL + RTOL |ref|)."""
    lines = []
    for (be, pname), rec in sorted(ERRORS.items()):
        lines.append("%s backend, %s pass: key, oracle distance, product's largest error (units of the fp32 bar)" % (be, pname))
        lines += ["  %-28s %10.4f %10.4f" % (k, a, c) for k, (a, c) in rec.items()]
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ fused step, state-side edges
def plant_state_edges(buf, g, csc=K.PUSH_INTERVAL - 3):
    """The state-side subset of the edges into primed buffers (rows 8 .. 83): see run_fused_state_edges."""
    import synth_common as SC
    SC.plant(buf, None, g, csc=csc)
    M = K.MAX_EPISODE_LENGTH
    ep = buf.episode_length.cpu()
    edges = [M - 2, M - 1, M, 799, 798, 1599, 0, 1, 30, 31, 32, 33, 62, 63]
    ep[8:8 + len(edges)] = torch.tensor(edges)
    buf.episode_length.copy_(ep)
    cmd = buf.view("commands").cpu().clone()
    for i, v in enumerate((F(0.1), up(0.1), dn(0.1), -F(0.1), -up(0.1))):
        cmd[40 + i, 0] = v
    for i, v in enumerate((3.0, -3.0, 0.0, -1e-7, 3.5, -3.5)):
        cmd[50 + i, 3] = v
    buf.view("commands").copy_(cmd)
    act = buf.view("actions").cpu().clone()
    act[60], act[61] = K.CLIP_ACTIONS, -K.CLIP_ACTIONS
    buf.view("actions").copy_(act)
    fat = buf.view("feet_air_time").cpu().clone()
    for i, v in enumerate((0.0, 1e-6, 0.49, 0.7)):
        fat[70 + i] = v
    buf.view("feet_air_time").copy_(fat)
    lc = buf.view("last_contacts").cpu().clone()
    lc[70:74:2], lc[71:74:2] = 1.0, 0.0
    buf.view("last_contacts").copy_(lc)
    ring = buf.obs_ring.cpu().clone()
    ring[80:84] = torch.tensor([40.0, -40.0]).repeat(ring[80:84].numel() // 2).view_as(ring[80:84])
    buf.obs_ring.copy_(ring)
    pring = buf.priv_ring.cpu().clone()
    pring[80:84, :, :72] = torch.tensor([-25.0, 25.0]).repeat(pring[80:84, :, :72].numel() // 2).view_as(pring[80:84, :, :72])
    buf.priv_ring.copy_(pring)


def run_fused_state_edges(buf, step, sync, g, seed, steps):
    """The fused step draws its own sim frame from Philox, so only the state side can be planted: episode lengths on the time-out,
    resample and gait edges, the step counter before the push interval, commands on the dead-band threshold and beyond the heading
    clamp, stored actions on the clip, foot timers on both sides of the air-time clamp, history rings holding frames beyond the
    observation clip.  `buf` is primed; step(actions) runs one fused step, sync() waits for it.  Compared with the oracle on the same
    Philox stream (synth_common.compare, low_speed flip budget unchanged).  Returns the event counts, the census of the sim-side edges
    the Philox frames happened to reach (information, not asserted) and the flips."""
    import synth_common as SC
    from oracle import synth_env_oracle as S
    N = buf.N
    flips = [0]
    plant_state_edges(buf, g)
    sync()
    o = SC.oracle_from_buffers(buf)
    counts = dict(reset=0, timeout=0, push=0)
    reached = dict(fz_over_1100=0, yr_over_50=0, gimbal=0, obs_beyond_clip=0, base_norm_between_01_and_1=0, feet_beyond_max_plus_half=0)
    for t in range(steps):
        a = torch.randn(N, 12, generator=g) * 1.5
        if t == 0:
            a[62], a[63] = 40.0, -40.0
        step(a)
        sync()
        _, _, _, _, info = S.synth_step(o, seed, a)
        SC.compare(buf, o, "step %d" % t, flips)
        if t == 0:      # the planted ring frames, clipped, are the older frames of the first stacked rows
            assert float(buf.obs[80:84].abs().max()) == K.CLIP_OBS and float(buf.priv_obs[80:84].abs().max()) == K.CLIP_OBS
        counts["reset"] += int(o.reset.sum())
        counts["timeout"] += int(o.time_out.sum())
        counts["push"] += int(info["pushed"])
        feet = list(K.FEET_BODIES)
        reached["fz_over_1100"] += int((o.sim.contact[:, feet].norm(dim=-1) > 1100).sum())
        jd = o.sim.dof_pos
        reached["yr_over_50"] += int((jd[:, :2].norm(dim=1) + jd[:, 6:8].norm(dim=1) > 50.1).sum())
        q = o.sim.root[:, 3:7]
        reached["gimbal"] += int(((2 * (q[:, 3] * q[:, 1] - q[:, 2] * q[:, 0])).abs() >= 1).sum())
        reached["obs_beyond_clip"] += int((o.obs[:, -K.NUM_SINGLE_OBS:].abs() > K.CLIP_OBS).any(1).sum())
        bn = o.sim.contact[:, K.BASE_BODY].norm(dim=-1)
        reached["base_norm_between_01_and_1"] += int(((bn > 0.1) & (bn <= 1.0)).sum())
        reached["feet_beyond_max_plus_half"] += int(((o.sim.rigid[:, feet[0], :2] - o.sim.rigid[:, feet[1], :2]).norm(dim=1) > K.MAX_DIST + 0.5).sum())
    return counts, reached, flips[0]


# ------------------------------------------------------------------------------------------------ generic options (monolithic chain only)
# Terrain map (custom origins, terrain curriculum, height measurements) and the command curriculum: legged_robot.py:400-431, 761-795.
# The command-curriculum decision is one per step, so its sides are passes: the resetting envs' mean tracking_lin_vel sum 1 % below and
# 1 % above 0.8 x scale x max_episode_length (23.04), and above it with the range one step from its cap.
GENERIC_PASSES = {
    "below the bar": dict(track=23.04 * 0.99, range0=None, expect=[-0.3, 0.6]),
    "above the bar": dict(track=23.04 * 1.01, range0=None, expect=[-0.8, 1.1]),
    "at the cap": dict(track=23.04 * 1.01, range0=[-1.2, 1.3], expect=[-1.5, 1.5]),
}
GENERIC_N, MAX_CURRICULUM = 44, 1.5
# name, what is planted: base xy (absolute, for the height-map cases; the map spans x in [-3, 43), y in [-3, 35)), quaternion;
# or, for the curriculum cases, the start level, the distance from the tile origin and the planar command norm (the env resets)
GENERIC_CASES = (
    [("heights inside", dict(xy=(12.34, 7.77)))] +
    [("heights beyond %s" % nm, dict(xy=xy)) for nm, xy in (("x low", (-10.26, 7.77)), ("x high", (60.34, 7.77)), ("y low", (12.34, -9.83)),
                                                              ("y high", (12.34, 50.77)), ("corner low low", (-10.26, -9.83)),
                                                              ("corner low high", (-10.26, 50.77)), ("corner high low", (60.34, -9.83)),
                                                              ("corner high high", (60.34, 50.77)))] +
    [("heights zero quaternion", dict(xy=(12.34, 7.77), quat=(0.0, 0.0, 0.0, 0.0))),
     ("heights quaternion scaled by 1e-12", dict(xy=(12.34, 7.77), quat=(0.1e-12, 0.05e-12, 0.3e-12, 1e-12))),
     ("promotion, distance above half a tile", dict(level=2, dist=4.1, cmd=0.3)),
     ("no move, distance below half a tile and above the command bar", dict(level=2, dist=3.9, cmd=0.3)),
     ("demotion, distance below the command bar", dict(level=2, dist=3.5, cmd=0.3)),
     ("no demotion, distance above the command bar", dict(level=2, dist=3.7, cmd=0.3)),
     ("promotion out of the top row", dict(level=4, dist=4.5, cmd=0.3)),
     ("demotion at level 0", dict(level=0, dist=1.0, cmd=0.3))])
NUM_GENERIC_CASES = 17
assert len(GENERIC_CASES) == NUM_GENERIC_CASES


def _yaw_apply64(q, v):
    """utils/math.py:39-43 (quat_apply_yaw) with isaacgym's normalize: x / norm.clamp(min = 1e-9)."""
    qy = q.copy()
    qy[:, :2] = 0.0
    n = np.sqrt(np.sum(qy ** 2, 1, keepdims=True))
    floor = n < F(1e-9)
    qy = qy / np.where(floor, F(1e-9), n)
    out = np.stack([_rot(qy, np.tile(v[p], (q.shape[0], 1))) for p in range(v.shape[0])], 1)
    return out, floor[:, 0]


def run_generic(backend, pass_name, sim_layout="soa"):
    """One planted step with the generic options on, at split = 0: the product against the fp32 oracle (compare_state: levels, origins'
    bits, sampled heights and the command range exact) and, on the case rows, against a float64 restatement of the height sampling,
    the level decision and the command-curriculum decision.  Returns the census {edge: {side: count}} of this pass."""
    gp = GENERIC_PASSES[pass_name]
    N = GENERIC_N
    g = torch.Generator().manual_seed(2718)
    fr, bm = 0.1 + 1.9 * torch.rand(N, 1, generator=g), 10.0 + 10.0 * torch.rand(N, 1, generator=g)
    spec = EC.random_terrain_spec(g, N)
    rows = torch.randperm(N, generator=g)[:NUM_GENERIC_CASES].tolist()
    for (name, c), i in zip(GENERIC_CASES, rows):
        if "level" in c:
            spec.levels[i] = c["level"]
    level0 = spec.levels.clone()
    o = XBotEnvOracle(N, frictions=fr, body_mass=bm, terrain=spec, command_curriculum=True, max_curriculum=MAX_CURRICULUM)
    env = EC.EnvUnderTest(backend, N, fr, bm, sim_layout=sim_layout, terrain=spec, command_curriculum=MAX_CURRICULUM)
    draws = (torch.rand(N, 12, generator=g), torch.rand(N, 3, generator=g), torch.randn(N, 47, generator=g), torch.rand(N, 2, generator=g),
             torch.randint(0, spec.max_level, (N,), generator=g))
    o.prime(*draws)
    env.prime(*draws)
    backend.sync()
    EC.compare_state(env, o, "generic prime")
    assert torch.equal(spec.levels, level0)
    # ---- plant
    ep = torch.randint(70, 700, (N,), generator=g)
    cmd = o.commands.clone()
    sums = torch.zeros(N, K.NUM_REWARDS)
    sums[:, K.REWARD_NAMES.index("tracking_lin_vel")] = gp["track"]
    frame = EC.synth_frames(g, N)
    root, contact = frame[0], frame[2].view(N, K.NUM_BODIES, 3)
    rad, ang = 3.0 * torch.rand(N, generator=g), 6.2831853 * torch.rand(N, generator=g)
    root[:, 0] = o.env_origins[:, 0] + rad * torch.cos(ang)
    root[:, 1] = o.env_origins[:, 1] + rad * torch.sin(ang)
    root[:, 2] += o.env_origins[:, 2]
    for (name, c), i in zip(GENERIC_CASES, rows):
        contact[i, BASE] = 0.0
        root[i, 3:7] = torch.tensor(c.get("quat", (0.0, 0.0, 0.0, 1.0)))
        if "xy" in c:
            root[i, 0:2] = torch.tensor(c["xy"])
        else:
            root[i, 0] = o.env_origins[i, 0] + c["dist"] * 0.6
            root[i, 1] = o.env_origins[i, 1] + c["dist"] * 0.8
            cmd[i, 0:2] = torch.tensor([0.0, c["cmd"]])
            contact[i, BASE] = torch.tensor([0.0, 0.0, 3.0])            # terminated: reset_idx runs the terrain curriculum
    csc = K.MAX_EPISODE_LENGTH - 1                                      # the step lands on the command-curriculum check (and on a push)
    o.ep_len, o.commands, o.episode_sums, o.common_step_counter = ep.clone(), cmd.clone(), sums.clone(), csc
    b = env.buf
    b.episode_length.copy_(ep); b.view("commands").copy_(cmd); b.view("episode_sums").copy_(sums); b.counters[L.CNT_STEP] = csc
    if gp["range0"] is not None:
        o.cmd_range_x = list(gp["range0"])
        b.command_range_x.copy_(torch.tensor(gp["range0"], dtype=torch.float64))
    a_in, nz = torch.randn(N, 12, generator=g), [torch.rand(N, generator=g), torch.randn(N, 12, generator=g), torch.rand(N, 6, generator=g),
                                                 torch.rand(N, 12, generator=g), torch.rand(N, 5, generator=g), torch.randn(N, 47, generator=g),
                                                 torch.rand(N, 2, generator=g), torch.randint(0, spec.max_level, (N,), generator=g)]
    origins_before = o.env_origins.clone()
    a_o = a_in.clone()
    o.pre_physics(a_o, nz[0], nz[1]); o.pd_torques(); o.sim.load(*frame); o.post_physics(*nz[2:])
    env.step(a_in, frame, *nz)
    EC.compare_state(env, o, "generic options, %s" % pass_name)
    assert o.cmd_range_x == gp["expect"], (o.cmd_range_x, gp["expect"])
    # ---- float64, case rows
    C = {}

    def add(edge, side, n):
        C.setdefault(edge, {}).setdefault(side, 0)
        C[edge][side] += int(n)
    w = lambda t: t.detach().cpu().double().numpy()
    R, q = w(root)[rows], w(root)[rows][:, 3:7]
    pts, floor = _yaw_apply64(q, w(spec.height_points))
    pts = (pts + R[:, None, :3] + F(spec.border_size)) / F(spec.hscale)
    ix, iy = np.trunc(pts[:, :, 0]).astype(np.int64), np.trunc(pts[:, :, 1]).astype(np.int64)
    nr, nc = spec.height_samples.shape
    px, py = np.clip(ix, 0, nr - 2), np.clip(iy, 0, nc - 2)
    hs = spec.height_samples.numpy().astype(np.int64)
    h64 = np.minimum(np.minimum(hs[px, py], hs[px + 1, py]), hs[px, py + 1]) * F(spec.vscale)
    got = w(b.measured_heights)[rows]
    hrows = [k for k, (name, c) in enumerate(GENERIC_CASES) if "xy" in c]
    assert np.array_equal(np.float32(h64[hrows]), np.float32(got[hrows])), "sampled heights vs float64"
    add("height map px", "clamped at 0", (ix[hrows] < 0).all(1).sum()); add("height map px", "clamped at rows - 2", (ix[hrows] > nr - 2).all(1).sum())
    add("height map py", "clamped at 0", (iy[hrows] < 0).all(1).sum()); add("height map py", "clamped at cols - 2", (iy[hrows] > nc - 2).all(1).sum())
    add("height map px", "inside", ((ix[hrows] >= 0) & (ix[hrows] <= nr - 2)).all(1).sum()); add("height map py", "inside", ((iy[hrows] >= 0) & (iy[hrows] <= nc - 2)).all(1).sum())
    add("height map corner", "both clamped", (((ix[hrows] < 0) | (ix[hrows] > nr - 2)) & ((iy[hrows] < 0) | (iy[hrows] > nc - 2))).all(1).sum())
    add("yaw quaternion norm", "below the 1e-9 floor", floor[hrows].sum()); add("yaw quaternion norm", "above it", (~floor[hrows]).sum())
    r_level = nz[7].numpy()
    for k, ((name, c), i) in enumerate(zip(GENERIC_CASES, rows)):
        if "level" not in c:
            continue
        d = float(np.sqrt(np.sum((R[k, :2] - w(origins_before)[i, :2]) ** 2)))
        bar_up, bar_down = F(spec.env_length / 2), float(np.sqrt(np.sum(w(cmd)[i, :2] ** 2))) * K.EPISODE_LENGTH_S * 0.5
        up_, down_ = d > bar_up, (d < bar_down) and not d > bar_up
        lv = c["level"] + int(up_) - int(down_)
        top = lv >= spec.max_level
        lv = int(r_level[i]) if top else max(lv, 0)
        assert bool(o.reset[i]) and int(b.terrain_levels[i]) == lv == int(spec.levels[i]), (name, lv, int(b.terrain_levels[i]))
        assert np.array_equal(w(b.view("env_origins"))[i], w(spec.origins)[lv, int(spec.types[i])]), name
        add("level promotion", "distance above half a tile" if up_ else "distance below half a tile", 1)
        if not up_:
            add("level demotion", "distance below the command bar" if down_ else "distance above the command bar", 1)
        add("level range", "out of the top row (random level)" if top else ("held at level 0" if c["level"] + int(up_) - int(down_) < 0 else "inside"), 1)
    m = w(o.reset)[:, None] if False else o.reset.numpy()
    k = K.REWARD_NAMES.index("tracking_lin_vel")
    moved = gp["track"] / float(K.MAX_EPISODE_LENGTH) > 0.8 * F(K.REWARD_SCALES_DT[k])      # this step's term (< 0.012) is far inside the 1 % margin
    assert bool(m.any()) and moved == (gp["expect"] != (gp["range0"] or [-0.3, 0.6]))
    add("command curriculum", "mean tracking sum above 0.8 x scale" if moved else "mean tracking sum below 0.8 x scale", 1)
    if moved:
        add("command curriculum cap", "binds" if gp["expect"][1] == MAX_CURRICULUM and gp["range0"] is not None else "does not bind", 1)
    assert [float(v) for v in b.command_range_x.cpu()] == gp["expect"]
    return C
