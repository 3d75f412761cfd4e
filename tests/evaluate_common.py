"""Shared by tests/test_evaluate.py (CPU) and tests/test_evaluate_gpu.py: the evaluation accumulator's arithmetic restated in numpy
float64 (what hgym_eval_accumulate must compute, include/hgym.h: HGYM_EVAL_*), and a hand-made trace with known answers."""
import numpy as np

SUMS, STEPS, ENV_STEPS, LIN_ERR, ANG_ERR, REWARD, EPISODES, TIMEOUTS, RETURN, LENGTH, TICKET, TERMS = 32, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
NUM_TERMS = 22


class EvalAccumulatorNp:
    """totals[32] float64 + per-env running return / length / previous episode sums, one add() per vec-step."""

    def __init__(self, n):
        self.n = n
        self.totals = np.zeros(SUMS, np.float64)
        self.cur_ret, self.cur_len = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self.prev_sums = np.zeros((NUM_TERMS, n), np.float64)

    def add(self, commands, lin_vel, ang_vel, episode_sums, rew, reset, time_out):
        """commands (4, n), lin_vel / ang_vel (3, n), episode_sums (22, n): the env-major state arrays AFTER the step; rew / reset /
        time_out (n,): the step's outputs."""
        f8 = lambda a: np.asarray(a, np.float32).astype(np.float64)
        c, lv, av, es, r = f8(commands), f8(lin_vel), f8(ang_vel), f8(episode_sums), f8(rew)
        done, to = np.asarray(reset).astype(bool), np.asarray(time_out).astype(bool)
        t = self.totals
        t[STEPS] += 1.0
        t[ENV_STEPS] += float(self.n)
        t[LIN_ERR] += np.sqrt((c[0] - lv[0]) ** 2 + (c[1] - lv[1]) ** 2).sum()
        t[ANG_ERR] += np.abs(c[2] - av[2]).sum()
        t[REWARD] += r.sum()
        ret, ln = self.cur_ret + r, self.cur_len + 1.0
        t[EPISODES] += float(done.sum())
        t[TIMEOUTS] += float((done & to).sum())
        t[RETURN] += ret[done].sum()
        t[LENGTH] += ln[done].sum()
        t[TERMS:TERMS + NUM_TERMS] += self.prev_sums[:, done].sum(axis=1)      # the sums as of the step before the episode's last
        self.cur_ret, self.cur_len = np.where(done, 0.0, ret), np.where(done, 0.0, ln)
        self.prev_sums = es.copy()


def hand_trace():
    """3 steps, 5 envs, two episode ends (env 2 at step 1 by time-out, env 4 at step 2 by a fall).  Every number is exactly
    representable, so the expected dict is known without rounding:
      env 0 is off its commanded planar velocity by (3, 4) -> 5 per step; every env is off its yaw command by 0.25;
      every env earns 0.5 (t + 1) at step t; reward term k stands at 0.125 (k + 1) (steps since the env's reset) after a step."""
    n, steps = 5, []
    since = np.zeros(n)
    for t in range(3):
        commands = np.zeros((4, n), np.float32)
        commands[0], commands[2] = 3.5, 0.5
        lin = np.zeros((3, n), np.float32)
        lin[0] = 3.5
        lin[0, 0], lin[1, 0] = 0.5, -4.0
        ang = np.zeros((3, n), np.float32)
        ang[2] = 0.25
        reset = np.zeros(n, bool)
        time_out = np.zeros(n, bool)
        if t == 1:
            reset[2] = time_out[2] = True
        if t == 2:
            reset[4] = True
        time_out[1] = t == 0                      # a time_out flag without a reset counts for nothing
        since = np.where(reset, 0.0, since + 1.0)
        sums = (0.125 * (np.arange(NUM_TERMS) + 1.0))[:, None] * since[None, :]
        steps.append(dict(commands=commands, lin_vel=lin, ang_vel=ang, episode_sums=sums.astype(np.float32),
                          rew=np.full(n, 0.5 * (t + 1), np.float32), reset=reset, time_out=time_out))
    return n, steps


def hand_trace_expected(reward_names, episode_length_s):
    exp = dict(episodes=2, mean_episode_return=(1.5 + 3.0) / 2, mean_episode_length=2.5, timeout_fraction=0.5, fall_fraction=0.5,
               mean_reward_per_step=1.0, lin_vel_tracking_error=5.0 * 3 / 15, ang_vel_tracking_error=0.25)
    for k, nm in enumerate(reward_names):
        # env 2 ends at step 1 with the sums of step 0 (0.125 (k + 1)), env 4 at step 2 with those of step 1 (0.25 (k + 1))
        exp["rew_" + nm] = 0.375 * (k + 1) / 2 / episode_length_s
    return exp
