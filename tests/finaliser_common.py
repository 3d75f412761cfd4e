"""The step finaliser (csrc/hgym_finalize.hpp) on planted inputs: a plain restatement of the reference's code in float32 CPU tensors
(RefFinaliser), the device harness that plants the same inputs and runs one of the finaliser's hosts through the C-ABI (Device), the
done patterns, and the comparison of everything the finaliser may write -- bit for bit.

The reference's code that RefFinaliser restates:
  * OnPolicyRunner.learn's book-keeping (on_policy_runner.py:143-156): ep_infos.append(infos["episode"]) every step; cur_reward_sum +=
    rewards, cur_episode_length += 1 (float32); new_ids = (dones > 0).nonzero() (ascending env ids); rewbuffer / lenbuffer (deque(maxlen=100))
    .extend(cur_*[new_ids]); cur_*[new_ids] = 0.
  * LeggedRobot.reset_idx (legged_robot.py:173-174, 199-210): extras["time_outs"] / extras["episode"] are re-assigned only when at least one
    env reset; extras["episode"][k] = mean over the reset envs of their episode sums / episode_length_s -- the kernels hand over the SUM
    (episode_acc) and the count, so the mean is episode_acc[k] / count, then / episode_length_s: two float32 divisions.
  * PPO.process_env_step (ppo.py:107-108): rewards + gamma * (values * time_outs) as three float32 roundings, and the dones.
Ring positions: slot (head + k) % 100 of log_stats' two rings holds the k-th episode appended from the head on -- what a deque(maxlen=100)
holds when written out as a circular buffer."""
import ctypes as C
from collections import deque

import torch

from hgym import _lib as L

F32 = torch.float32
RING = L.LOG_RING


def f32(x):
    return torch.tensor(x, dtype=F32)


def same_bits(a, b):
    """Bit equality (so a NaN sentinel the kernel left, or a -0.0, shows); integer tensors by value."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape:
        return False
    if a.dtype == F32 and b.dtype == F32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a.to(torch.int64), b.to(torch.int64))


# ---------------------------------------------------------------------------------------------------------------- planted inputs
class Plan:
    """Everything planted before the first call and before every call of one sequence -- shared by the reference and the device."""

    def __init__(self, N, masks, counts, seed, ncustom=0, head=97, fill=37):
        g = torch.Generator().manual_seed(seed)
        self.N, self.masks, self.counts, self.ncustom = N, masks, counts, ncustom
        self.gamma = 0.994
        r = lambda *s: torch.randn(*s, generator=g)
        # state carried from call to call
        self.extras_time_outs0 = torch.rand(N, generator=g) < 0.5
        self.extras_episode0 = r(L.NUM_REWARDS)
        self.extras_custom0 = r(max(ncustom, 1))
        self.log_cur0 = torch.stack([r(N) * 3, torch.randint(0, 2400, (N,), generator=g).float()])
        ls = torch.full((L.LOG_STATS,), -7.0)
        ls[L.LOG_TERMS:L.LOG_TERMS + L.NUM_REWARDS] = r(L.NUM_REWARDS)
        ls[L.LOG_STEPS] = 5.0
        ls[L.LOG_RING_HEAD], ls[L.LOG_RING_FILL] = float(head), float(fill)
        ls[L.LOG_RETURNS:L.LOG_RETURNS + RING] = -1000.0 - torch.arange(RING).float()         # a slot nobody wrote shows
        ls[L.LOG_LENGTHS:L.LOG_LENGTHS + RING] = -2000.0 - torch.arange(RING).float()
        self.log_stats0 = ls
        self.counters0 = torch.tensor([1234, 0, 77, 5], dtype=torch.int64)
        self.t_step0 = 41
        # fresh for every call
        self.calls = []
        for m, cnt in zip(masks, counts):
            assert m.shape == (N,) and m.dtype == torch.bool
            self.calls.append(dict(reset=m, count=int(cnt), rew=r(N), time_out=torch.rand(N, generator=g) < 0.4, values=r(N) * 2,
                                   episode_acc=r(24) * 50, custom_acc=r(max(ncustom, 1)) * 50))


# ---------------------------------------------------------------------------------------------------------------- done patterns
def _ids(N, ids):
    m = torch.zeros(N, dtype=torch.bool)
    ids = [i for i in ids if 0 <= i < N]
    if ids:
        m[torch.tensor(ids)] = True
    return m


def _spread(N, k, g, lo=0, hi=None):
    """k distinct envs of [lo, hi), random."""
    hi = N if hi is None else hi
    k = min(k, hi - lo)
    return _ids(N, (lo + torch.randperm(hi - lo, generator=g)[:k]).tolist())


def dense_sequence(N, seed):
    """The done masks of one sequence, in call order.  A lane of the general form (fin_log) owns env `row + lane`: env 63 is lane 63 of
    wavefront 0, env 64 lane 0 of wavefront 1.  A lane of the one-pass form (fin_log_fused) owns 8 consecutive envs: envs 504..511 are
    lane 63 of wavefront 0, envs 512..519 lane 0 of wavefront 1.  Patterns that need more envs than N has are left out."""
    g = torch.Generator().manual_seed(seed)
    seq = [("none", _ids(N, [])), ("env 0", _ids(N, [0])), ("env N-1", _ids(N, [N - 1]))]
    for i in (63, 64, 511, 512):
        if i < N:
            seq.append(("env %d" % i, _ids(N, [i])))
    if N >= 128:
        seq.append(("wavefront 1 of the general form", _ids(N, range(64, 128))))
    if N >= 1024:
        seq.append(("wavefront 1 of the one-pass form", _ids(N, range(512, 1024))))
    seq.append(("one in every 64 envs", _ids(N, [w + (5 * (w // 64) + 3) % 64 for w in range(0, N, 64)])))
    if N > 512:
        seq.append(("one in every 512 envs", _ids(N, [w + (37 * (w // 512) + 11) % 512 for w in range(0, N, 512)])))
    seq += [("60", _spread(N, 60, g)), ("60 again: the head wraps", _spread(N, 60, g))]
    if N >= 100:
        seq.append(("exactly 100", _spread(N, 100, g)))
    if N >= 101:
        seq.append(("exactly 101", _spread(N, 101, g)))
    seq.append(("none", _ids(N, [])))
    seq.append(("all N", torch.ones(N, dtype=torch.bool)))
    if N > 1024:
        # more than 100 split over the rows / trips: 80 + 70 in the first two thirds, then the last 8 envs (for N = 4104 / 8200 the single
        # live lane of the second trip on 512 / 1024 lanes) and 52 more in the last third: the later ones overwrite survivors of the earlier
        third = N // 3
        m = _spread(N, 80, g, 0, third) | _spread(N, 70, g, third, 2 * third) | _spread(N, 52, g, 2 * third, N - 8) | _ids(N, range(N - 8, N))
        seq.append(("210 over the rows", m))
        m = _spread(N, 120, g, 0, min(N - 8, 4096)) | _ids(N, range(N - 5, N))
        seq.append(("120 early, 5 in the last lane", m))
    seq.append(("Bernoulli(0.3)", torch.rand(N, generator=g) < 0.3))
    seq.append(("Bernoulli(0.3) again", torch.rand(N, generator=g) < 0.3))
    return seq


def sparse_sequence(N):
    """Fewer than 100 finished episodes in the whole sequence: the rings never fill."""
    seq = [("none", _ids(N, [])), ("env 0", _ids(N, [0])), ("env N-1", _ids(N, [N - 1])), ("envs 63, 64", _ids(N, [63, 64])),
           ("envs 511, 512", _ids(N, [511, 512])), ("none", _ids(N, [])), ("a few", _ids(N, range(3, N, max(N // 9, 1)))),
           ("env 0 again", _ids(N, [0]))]
    assert sum(int(m.sum()) for _, m in seq) < 100
    return seq


def reset_counts(n, N):
    """The planted counters[CNT_RESETS] of n calls: zero on every third call (nothing may be refreshed), else varied positive."""
    pos = [1, 3, N, 7, 2 * N + 1]
    return [0 if k % 3 == 1 else pos[k % len(pos)] for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------- the reference
class RefFinaliser:
    """sink: "immediate" (t_values set), "deferred" (t_values NULL, t_time_outs set) or None; log: the logging sink is bound;
    defer: HgymEnvOut.defer_finalize (someone else bumps t_step); count_external: the host keeps the reset count and the episode
    accumulators outside HgymEnvState (hgym_rollout_end: its scratch block, zero here), so the count is 0 on every call."""

    def __init__(self, plan, episode_length_s, sink="immediate", log=True, defer=False, count_external=False):
        p = self.plan = plan
        self.N, self.sink, self.log, self.defer, self.count_external = p.N, sink, log, defer, count_external
        self.els = f32(episode_length_s)
        self.extras_time_outs = p.extras_time_outs0.clone()
        self.extras_episode = p.extras_episode0.clone()
        self.extras_custom = p.extras_custom0.clone()
        self.cur_reward_sum, self.cur_episode_length = p.log_cur0[0].clone(), p.log_cur0[1].clone()
        self.log_stats = p.log_stats0.clone()
        self.counters = p.counters0.clone()
        self.t_step = p.t_step0
        head, fill = int(p.log_stats0[L.LOG_RING_HEAD]), int(p.log_stats0[L.LOG_RING_FILL])
        order = [(head - fill + k) % RING for k in range(fill)]            # what the planted ring holds, oldest first
        self.rewbuffer = deque((float(p.log_stats0[L.LOG_RETURNS + s]) for s in order), maxlen=RING)
        self.lenbuffer = deque((float(p.log_stats0[L.LOG_LENGTHS + s]) for s in order), maxlen=RING)

    def call(self, k):
        c, N = self.plan.calls[k], self.N
        cnt = 0 if self.count_external else c["count"]
        self.episode_acc, self.custom_acc = c["episode_acc"].clone(), c["custom_acc"].clone()
        # reset_idx: only when an env reset
        if cnt > 0:
            n = f32(float(cnt))
            self.extras_episode = self.episode_acc[:L.NUM_REWARDS] / n / self.els
            self.episode_acc[:L.NUM_REWARDS] = 0.0
            if self.plan.ncustom:
                K = self.plan.ncustom
                self.extras_custom[:K] = self.custom_acc[:K] / n / self.els
                self.custom_acc[:K] = 0.0
            self.extras_time_outs = c["time_out"].clone()
        # process_env_step
        nan, seven = torch.full((N,), float("nan")), torch.full((N,), 7, dtype=torch.uint8)
        self.t_rewards, self.t_dones, self.t_time_outs = nan, seven.clone(), seven.clone()
        if self.sink == "immediate":
            boot = c["values"] * self.extras_time_outs.float()
            gb = f32(self.plan.gamma) * boot
            self.t_rewards = c["rew"] + gb
            self.t_dones = c["reset"].to(torch.uint8)
        elif self.sink == "deferred":
            self.t_rewards = c["rew"].clone()
            self.t_dones = c["reset"].to(torch.uint8)
            self.t_time_outs = self.extras_time_outs.to(torch.uint8)
        # the runner's book-keeping
        if self.log:
            ls = self.log_stats
            ls[L.LOG_TERMS:L.LOG_TERMS + L.NUM_REWARDS] += self.extras_episode          # ep_infos.append(infos["episode"]), summed
            ls[L.LOG_STEPS] += 1.0
            self.cur_reward_sum += c["rew"]
            self.cur_episode_length += 1
            new_ids = (c["reset"] > 0).nonzero(as_tuple=False)
            self.rewbuffer.extend(self.cur_reward_sum[new_ids][:, 0].numpy().tolist())
            self.lenbuffer.extend(self.cur_episode_length[new_ids][:, 0].numpy().tolist())
            head, fill = int(ls[L.LOG_RING_HEAD]), int(ls[L.LOG_RING_FILL])
            for i in new_ids[:, 0].tolist():                                            # the same appends, as a circular buffer
                ls[L.LOG_RETURNS + head], ls[L.LOG_LENGTHS + head] = self.cur_reward_sum[i], self.cur_episode_length[i]
                head, fill = (head + 1) % RING, min(fill + 1, RING)
            ls[L.LOG_RING_HEAD], ls[L.LOG_RING_FILL] = float(head), float(fill)
            self.cur_reward_sum[new_ids] = 0
            self.cur_episode_length[new_ids] = 0
        # counters
        if self.sink is not None and not self.defer:
            self.t_step += 1
        if not self.count_external:
            self.counters[L.CNT_RESETS] = 0
        self.counters[L.CNT_STEP] += 1
        self.counters[L.CNT_RING] += 1


# ---------------------------------------------------------------------------------------------------------------- the device
DEVICE = "cuda"
RIDE_ROWS = 32          # hgym_policy_act_fin's M: 2 nets x ceil(32 / 32) tiles <= CUs -> launch_fwd<32, 8, 4>: 8 wavefronts = 512 lanes
_ride_net = None


def ride_net():
    """A small net on the fused bf16 path (only there does the finaliser ride in mlp_fwd_kernel; elsewhere it is fin_only_kernel)."""
    global _ride_net
    if _ride_net is None:
        from hgym import NetBuffers, make_net_config
        net = NetBuffers(make_net_config(188, 146, 12, [256, 256, 256], [256, 256, 256], "bf16", 64), "cuda")
        assert net.shadow_ld(0) > 0 and net.shadow_ld(1) > 0, "not the fused path"
        net.views["std"].fill_(1.0)
        net.sync_shadow()
        e = lambda *s: torch.zeros(*s, device="cuda")
        io = dict(obs=e(RIDE_ROWS, 188), priv=e(RIDE_ROWS, 146), step=torch.zeros(1, dtype=torch.int64, device="cuda"),
                  out=dict(actions=e(RIDE_ROWS, 12), mu=e(RIDE_ROWS, 12), sigma=e(RIDE_ROWS, 12), logp=e(RIDE_ROWS), values=e(RIDE_ROWS, 1)))
        _ride_net = (net, io)
    return _ride_net


def lanes_of(host, N):
    """The finaliser workgroup's width on each host."""
    return {"finalize": 1024 if N > 256 else 256, "ride512": 512, "rollout_end": 1024 if N > 256 else 256}[host]


class Device:
    """host: "finalize" (hgym_env_finalize: env_finalize_kernel, 256 lanes up to 256 envs, 1024 above), "ride512" (hgym_policy_act_fin on
    the fused path with 32 rows: the extra workgroup of mlp_fwd_kernel<32, 8, 4, true>, 512 lanes) or "rollout_end" (hgym_rollout_end:
    rollout_fin_kernel; the reset count and the accumulators live in the caller's zero-filled scratch block).
    misalign: None, or "rew" / "reset" / "log_cur": that column is a view one element into its allocation."""

    def __init__(self, plan, host, sink="immediate", log=True, defer=False, misalign=None):
        from hgym import EnvBuffers, default_env_config
        p = self.plan = plan
        N = self.N = p.N
        self.host, self.sink_kind, self.log = host, sink, log
        cfg = self.cfg = default_env_config(N)
        buf = self.buf = EnvBuffers(cfg, DEVICE)
        buf.log_sink = log
        if p.ncustom:
            buf.set_custom_rewards(list(range(p.ncustom)))
        self.rew, self.reset, self.log_cur = buf.rew, buf.reset, buf.log_cur
        if misalign == "rew":
            self.rew = torch.zeros(N + 1, device=DEVICE)[1:]
        elif misalign == "reset":
            self.reset = torch.zeros(N + 1, dtype=torch.uint8, device=DEVICE)[1:]
        elif misalign == "log_cur":
            self.log_cur = torch.zeros(2 * N + 1, device=DEVICE)[1:].view(2, N)
        else:
            assert misalign is None
        self.sink = None
        if sink is not None:
            self.sink = dict(values=torch.zeros(N, device=DEVICE) if sink == "immediate" else None, rewards=torch.zeros(N, device=DEVICE),
                             dones=torch.zeros(N, dtype=torch.uint8, device=DEVICE), time_outs=torch.zeros(N, dtype=torch.uint8, device=DEVICE),
                             step=torch.full((1,), p.t_step0, dtype=torch.int64, device=DEVICE), gamma=p.gamma)
        self.st = buf.state_struct()
        self.out = buf.out_struct(sink=self.sink, defer_finalize=defer)
        self.out.rew, self.out.reset = L.fptr(self.rew), L.u8ptr(self.reset)
        if log:
            self.out.log_cur = L.fptr(self.log_cur)
        for name, a in (("rew", 16), ("reset", 8), ("log_cur", 16)):
            assert (getattr(self, name).data_ptr() % a != 0) == (misalign == name)
        buf.extras_time_outs.copy_(p.extras_time_outs0)
        buf.extras_episode.copy_(p.extras_episode0)
        if p.ncustom:
            buf.extras_custom.copy_(p.extras_custom0)
        self.log_cur.copy_(p.log_cur0)
        buf.log_stats.copy_(p.log_stats0)
        buf.counters.copy_(p.counters0)

    def call(self, k):
        c, buf, p = self.plan.calls[k], self.buf, self.plan
        self.rew.copy_(c["rew"])
        self.reset.copy_(c["reset"])
        buf.time_out.copy_(c["time_out"])
        buf.episode_acc.copy_(c["episode_acc"])
        if p.ncustom:
            buf.custom_acc.copy_(c["custom_acc"])
        if self.host != "rollout_end":
            buf.counters[L.CNT_RESETS] = c["count"]
        if self.sink is not None:
            if self.sink["values"] is not None:
                self.sink["values"].copy_(c["values"])
            self.sink["rewards"].fill_(float("nan"))
            self.sink["dones"].fill_(7)
            self.sink["time_outs"].fill_(7)
        self.launch()

    def launch(self):
        buf = self.buf
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.host == "finalize":
            L.check(L.lib.hgym_env_finalize(C.byref(self.cfg), C.byref(self.st), C.byref(self.out), s), "hgym_env_finalize")
        elif self.host == "ride512":
            net, io = ride_net()
            net.act(io["obs"], io["priv"], seed=3, step_counter=io["step"], out=io["out"], env_fin=(self.cfg, self.st, self.out))
        elif self.host == "rollout_end":
            L.check(L.lib.hgym_rollout_end(C.byref(self.cfg), C.byref(self.st), C.byref(self.out), C.c_void_p(buf.rollout_scratch.data_ptr()),
                                           0, s), "hgym_rollout_end")
        else:
            raise ValueError(self.host)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the comparison
def ring_in_order(ls):
    """The two rings of a log_stats vector as lists, oldest episode first, from its own head and fill."""
    head, fill = int(ls[L.LOG_RING_HEAD]), int(ls[L.LOG_RING_FILL])
    slots = [(head - fill + k) % RING for k in range(fill)]
    return [float(ls[L.LOG_RETURNS + s]) for s in slots], [float(ls[L.LOG_LENGTHS + s]) for s in slots]


def compare(ref, d, k, what):
    """Everything one call may have written, and the inputs it must not write -- bit for bit."""
    c, buf, p = ref.plan.calls[k], d.buf, ref.plan
    tag = lambda name: "%s, call %d (%s): %s" % (what, k, c.get("name", ""), name)
    assert same_bits(buf.extras_time_outs.to(torch.uint8), ref.extras_time_outs.to(torch.uint8)), tag("extras_time_outs (all N bytes)")
    assert same_bits(buf.extras_episode, ref.extras_episode), tag("extras_episode")
    if d.host != "rollout_end":
        assert same_bits(buf.episode_acc, ref.episode_acc), tag("episode_acc")
    if p.ncustom:
        assert same_bits(buf.extras_custom, ref.extras_custom), tag("extras_custom")
        assert same_bits(buf.custom_acc, ref.custom_acc), tag("custom_acc")
    if d.sink is not None:
        assert same_bits(d.sink["rewards"], ref.t_rewards), tag("t_rewards")
        assert same_bits(d.sink["dones"], ref.t_dones), tag("t_dones")
        assert same_bits(d.sink["time_outs"], ref.t_time_outs), tag("t_time_outs")
        assert int(d.sink["step"][0]) == ref.t_step, tag("t_step")
        if d.sink["values"] is not None:
            assert same_bits(d.sink["values"], c["values"]), tag("t_values (an input)")
    assert buf.counters.cpu().tolist() == ref.counters.tolist(), tag("counters %s" % buf.counters.cpu().tolist())
    ls = buf.log_stats.cpu()
    if d.log:
        ring_r, ring_l = ring_in_order(ls)
        assert (int(ls[L.LOG_RING_HEAD]), int(ls[L.LOG_RING_FILL])) == (int(ref.log_stats[L.LOG_RING_HEAD]), int(ref.log_stats[L.LOG_RING_FILL])), \
            tag("ring head / fill")
        assert ring_r == list(ref.rewbuffer), tag("returns ring, in order from the head, against the deque")
        assert ring_l == list(ref.lenbuffer), tag("lengths ring, in order from the head, against the deque")
    assert same_bits(ls, ref.log_stats), tag("log_stats %s" % (ls.view(torch.int32) != ref.log_stats.view(torch.int32)).nonzero().flatten().tolist())
    assert same_bits(d.log_cur[0], ref.cur_reward_sum), tag("log_cur returns")
    assert same_bits(d.log_cur[1], ref.cur_episode_length), tag("log_cur lengths")
    assert same_bits(d.rew, c["rew"]) and same_bits(d.reset.to(torch.uint8), c["reset"].to(torch.uint8)), tag("rew / reset (inputs)")
    assert same_bits(buf.time_out.to(torch.uint8), c["time_out"].to(torch.uint8)), tag("time_out (an input)")


def snapshot(d):
    """What a later run with other pointer alignments has to reproduce."""
    buf = d.buf
    out = [buf.extras_time_outs.to(torch.uint8), buf.extras_episode, buf.episode_acc, buf.counters, buf.log_stats, d.log_cur]
    if d.sink is not None:
        out += [d.sink["rewards"], d.sink["dones"], d.sink["time_outs"], d.sink["step"]]
    return [t.detach().cpu().clone() for t in out]


def make_plan(N, seq, seed, ncustom=0, head=97, fill=37, counts=None):
    plan = Plan(N, [m for _, m in seq], reset_counts(len(seq), N) if counts is None else counts, seed, ncustom=ncustom, head=head, fill=fill)
    for c, (name, _) in zip(plan.calls, seq):
        c["name"] = name
    return plan


def run_sequence(plan, host, sink="immediate", log=True, defer=False, misalign=None, what=""):
    """Plant, call and compare, call after call; -> the device's snapshots."""
    ref = RefFinaliser(plan, default_episode_length_s(plan.N), sink=sink, log=log, defer=defer, count_external=host == "rollout_end")
    d = Device(plan, host, sink=sink, log=log, defer=defer, misalign=misalign)
    snaps = []
    for k in range(len(plan.calls)):
        ref.call(k)
        d.call(k)
        compare(ref, d, k, what or "%s, N = %d" % (host, plan.N))
        snaps.append(snapshot(d))
    return ref, d, snaps


def default_episode_length_s(N):
    from hgym import default_env_config
    return float(default_env_config(N).episode_length_s)
