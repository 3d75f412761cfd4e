"""-m gpu: the step finaliser (csrc/hgym_finalize.hpp: fin_fused / fin_part1 + fin_store, fin_log_fused / fin_log, the counters) on
PLANTED inputs through the C-ABI, call after call, against the reference's own few lines of Python restated in float32 on the CPU
(tests/finaliser_common.py) -- every comparison bit for bit, the two 100-entry rings slot by slot from the known head.

No tolerance anywhere: every device operation here is a copy, one fp32 add in a fixed per-env order, the three fp32 roundings of the
stored reward (contraction off in the source), or an fp32 division -- and hipcc's fp32 division is the correctly rounded one (build.py
passes neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt), so the two divisions of extras["episode"] equal torch's.

The hosts and their workgroup widths:
  finalize     hgym_env_finalize -> env_finalize_kernel: 256 lanes for N <= 256, 1024 lanes above.
  ride512      hgym_policy_act_fin on the fused bf16 path with M = 32 rows: 2 nets x ceil(32 / 32) tiles fit the chip, so
               launch_fwd<32, 8, 4> -> the extra workgroup of mlp_fwd_kernel<32, 8, 4, true>: 8 wavefronts = 512 lanes (the width
               of rollout_step_kernel's finaliser workgroup, RO_NT).
  rollout_end  hgym_rollout_end -> rollout_fin_kernel (1024 lanes above 256 envs).  It takes the reset count and the episode
               accumulators from the rollout's scratch block, which only a rollout's own steps fill: without opening a whole rollout
               only the count-0 branch can be planted (a zero-filled block).  That branch is run here; the rest is the same fin_block at
               1024 lanes as `finalize`, and tests/test_runner_gpu.py runs it inside real rollouts.

Which form each env count reaches (general: fin_part1 + fin_store + fin_log; one-pass: fin_fused + fin_log_fused, a lane owns 8 envs):
      N   finalize                                      ride512 (512 lanes)
      8   one-pass, one lane of 256                     one-pass, one lane
     37   general, one partial wavefront                general
    250   general, 256 lanes, dones in 4 wavefronts     general
    256   one-pass, 256 lanes                           one-pass
    264   one-pass, 1024 lanes, 33 lanes busy           one-pass
   1001   general, one row of 1024 lanes                general, two rows
   2500   general, three rows, the last ragged          general, five rows
   4096   one-pass, one trip                            one-pass, one trip (512 lanes x 8 envs)
   4104   one-pass, one trip                            one-pass, SECOND trip with a single live lane
   8192   one-pass, one trip (1024 lanes x 8 envs)      one-pass, two full trips
   8200   one-pass, SECOND trip with a single live lane one-pass, three trips
"""
import pytest
import torch

import finaliser_common as FC
from hgym import _lib as L

pytestmark = pytest.mark.gpu

ENV_COUNTS = [8, 37, 250, 256, 264, 1001, 2500, 4096, 4104, 8192, 8200]
HOSTS = ["finalize", "ride512"]


@pytest.mark.parametrize("N", ENV_COUNTS)
@pytest.mark.parametrize("host", HOSTS)
def test_dense_done_patterns_call_after_call(host, N):
    """One sequence of consecutive calls per (host, N) with the immediate transition sink and the logging sink bound.  Done masks, in
    order: none; exactly one (env 0, env N - 1, envs 63 / 64 / 511 / 512: lane 63 of a wavefront and lane 0 of the next in either form);
    a whole wavefront and nothing else; one in every wavefront; 60 + 60 (the head wraps); exactly 100; exactly 101; none; all N;
    more than 100 split over the rows / trips so that later rows overwrite survivors of earlier ones; Bernoulli(0.3) twice.  The rings
    start at head 97 with 37 entries and known contents, so they wrap, saturate and are overwritten with known values.
    counters[CNT_RESETS] is 0 on every third call while time_out differs from the stale extras["time_outs"]: nothing may be refreshed,
    the stored reward uses the STALE flags, extras["episode"] / episode_acc stay, LOG_TERMS still adds the unchanged extras["episode"].
    Every one of the N time-out bytes is compared after every call (a late wavefront of a 1024-lane workgroup that read the cleared
    count would keep stale ones)."""
    seq = FC.dense_sequence(N, seed=1000 + N)
    assert len(seq) >= 6
    plan = FC.make_plan(N, seq, seed=N)
    assert 0 in plan.counts and max(plan.counts) > 0
    ref, d, _ = FC.run_sequence(plan, host)
    fill = min(L.LOG_RING, 37 + sum(int(m.sum()) for _, m in seq))
    assert len(ref.rewbuffer) == fill == int(d.buf.log_stats[L.LOG_RING_FILL]) and (fill == L.LOG_RING or N == 8)
    assert ref.t_step == plan.t_step0 + len(seq)
    assert FC.lanes_of(host, N) == (512 if host == "ride512" else 256 if N <= 256 else 1024)


@pytest.mark.parametrize("N", [37, 264, 2500, 8192])
@pytest.mark.parametrize("host", HOSTS)
def test_fewer_than_a_ring_of_episodes(host, N):
    """Fewer than 100 episodes finish in the whole sequence, from empty rings: LOG_RING_FILL stays below 100, slot k holds the k-th
    episode, and log_stats_summary hands out exactly the filled part, in order; every reset count positive."""
    from hgym import log_stats_summary
    seq = FC.sparse_sequence(N)
    plan = FC.make_plan(N, seq, seed=7 * N, head=0, fill=0, counts=[1 + k for k in range(len(seq))])
    ref, d, _ = FC.run_sequence(plan, host)
    total = sum(int(m.sum()) for _, m in seq)
    ls = d.buf.log_stats.cpu()
    assert 0 < total < L.LOG_RING and int(ls[L.LOG_RING_FILL]) == total == int(ls[L.LOG_RING_HEAD]) == len(ref.rewbuffer)
    terms = ["t%d" % k for k in range(L.NUM_REWARDS)]
    ep, returns, lengths = log_stats_summary(ls, terms, terms)
    assert returns == list(ref.rewbuffer) and lengths == list(ref.lenbuffer)
    steps = 5.0 + len(seq)
    assert ep == {"rew_" + n: float(ref.log_stats[L.LOG_TERMS + k]) / steps for k, n in enumerate(terms)}


@pytest.mark.parametrize("N", [264, 1001])
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("sink,log,defer", [("deferred", True, False), (None, True, False), ("immediate", False, False),
                                            ("immediate", True, True), ("deferred", False, True), (None, False, False)])
def test_sink_kinds(host, N, sink, log, defer):
    """The transition sink of the deferred kind (t_values NULL, t_time_outs set: raw reward + the bootstrap's flags; an immediate sink
    never touches t_time_outs, which keeps its sentinel), no sink at all (only the extras and the counters move, t_step stays), the logging
    sink off (log_cur and log_stats keep their planted values), and defer_finalize = 1 (t_step is not this call's to bump) -- in the
    one-pass form (264) and the general one (1001)."""
    seq = FC.dense_sequence(N, seed=N)[:9]
    plan = FC.make_plan(N, seq, seed=3 * N + 1)
    ref, d, _ = FC.run_sequence(plan, host, sink=sink, log=log, defer=defer)
    assert ref.t_step == plan.t_step0 + (len(seq) if (sink is not None and not defer) else 0)
    if not log:
        assert FC.same_bits(d.buf.log_stats, plan.log_stats0) and FC.same_bits(d.log_cur, plan.log_cur0)


@pytest.mark.parametrize("N", [256, 4096])
@pytest.mark.parametrize("host", HOSTS)
def test_misaligned_columns_take_the_general_forms(host, N):
    """N % 8 == 0 but rew, reset or log_cur one element into its allocation (4, 1, 4 bytes off): the one-pass forms test the pointers and
    decline (fin_fused for rew / reset under a sink, fin_log_fused for all three), the general forms run -- and give the reference's bits,
    which are also the aligned run's.  (That the one-pass form declined is not visible from outside; what is checked is the result.)"""
    seq = FC.dense_sequence(N, seed=N + 5)
    seq = seq[:4] + seq[-6:]
    plan = FC.make_plan(N, seq, seed=N + 9)
    _, _, aligned = FC.run_sequence(plan, host)
    for column in ("rew", "reset", "log_cur"):
        _, _, other = FC.run_sequence(plan, host, misalign=column, what="%s, N = %d, %s misaligned" % (host, N, column))
        for k, (a, b) in enumerate(zip(aligned, other)):
            for x, y in zip(a, b):
                assert FC.same_bits(x, y), (column, k)


@pytest.mark.parametrize("host", HOSTS)
def test_custom_reward_terms(host):
    """num_custom_rewards = 3 with custom_acc / extras_custom bound, N = 264: the user-defined terms' means are refreshed and their
    accumulators cleared under the same reset-count rule as the built-in ones (and left alone when no env reset)."""
    N = 264
    seq = FC.dense_sequence(N, seed=11)[:8]
    plan = FC.make_plan(N, seq, seed=12, ncustom=3)
    ref, d, _ = FC.run_sequence(plan, host)
    assert int(d.cfg.num_custom_rewards) == 3 and 0 in plan.counts and max(plan.counts) > 0
    assert not FC.same_bits(ref.extras_custom, plan.extras_custom0)


@pytest.mark.parametrize("N", [2500, 8200])
def test_rollout_end_without_a_reset(N):
    """hgym_rollout_end on a zero-filled scratch block (reset count 0, see the module docstring): rollout_fin_kernel at 1024 lanes --
    nothing refreshed, the stored reward on the stale flags, the whole of the logging book-keeping, the step counters + 1, and
    counters[CNT_RESETS] (not this host's reset count) left as planted."""
    seq = FC.dense_sequence(N, seed=N + 1)
    seq = seq[:3] + seq[-6:]
    plan = FC.make_plan(N, seq, seed=N + 2, counts=[0] * len(seq))
    plan.counters0[L.CNT_RESETS] = 9
    ref, d, _ = FC.run_sequence(plan, "rollout_end")
    assert int(d.buf.counters[L.CNT_RESETS]) == 9 and FC.same_bits(d.buf.extras_time_outs.to(torch.uint8), plan.extras_time_outs0.to(torch.uint8))
    assert int(d.buf.rollout_scratch.view(torch.int64)[:8 * 8].abs().sum()) == 0          # the block's header: still zero
