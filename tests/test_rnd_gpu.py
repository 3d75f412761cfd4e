"""-m gpu: hgym_rnd_rewards against the float64 restatement of tests/rnd_common.py.

Bars.  err: (K + 2) * 2^-24 relative to the exact value -- the bound of a K-term fp32 sum of non-negative terms plus one square root.
G, mean, var: 1e-10 relative, continued from the device's own fp32 errors -- an ordered fp64 sum of under 10^4 terms is good to about
10^-12; two decades of margin.  intrinsic and rewards: BITWISE, intrinsic = fp32(err_gpu * scale) with scale recomputed in fp64 from the
device's own std and the schedule, rewards = fp32(rewards_in + intrinsic)."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard_common as G
import rnd_common as R
from hgym import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cfg(gamma=0.99, normalize=True, schedule=R.CONSTANT, w0=1.0, final_value=0.0, initial_step=0, final_step=0):
    return L.RndConfig(gamma, w0, final_value, initial_step, final_step, schedule, 1 if normalize else 0)


def _sched(cfg):
    return dict(schedule=cfg.schedule, w0=cfg.weight, final_value=cfg.final_value, initial_step=cfg.initial_step, final_step=cfg.final_step)


def _inputs(T, n, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, n, K, generator=g), torch.randn(T, n, K, generator=g), torch.randn(T, n, generator=g))


def _run(T, n, K, pred, target, rewards, cfg, block, alloc=None):
    """One call on device copies; -> dict of host numpy arrays (err, intrinsic, rewards, block)."""
    put = (lambda t: t.to(DEV)) if alloc is None else alloc.place
    new = (lambda *s: torch.empty(*s, device=DEV)) if alloc is None else (lambda *s: alloc.carve(s, F32))
    p, q, r = put(pred.to(DEV)), put(target.to(DEV)), put(rewards.to(DEV))
    err, intr = new(T, n), new(T, n)
    L.check(L.lib.hgym_rnd_rewards(T, n, K, L.fptr(p), L.fptr(q), L.fptr(r), L.fptr(err), L.fptr(intr), C.byref(cfg), L.f64ptr(block), _s()),
            "hgym_rnd_rewards")
    torch.cuda.synchronize()
    return dict(err=err.cpu().numpy(), intrinsic=intr.cpu().numpy(), rewards=r.cpu().numpy(), block=block.cpu().numpy().copy())


def _state_of(block, n):
    return dict(mean=float(block[R.MEAN]), var=float(block[R.VAR]), count=float(block[R.COUNT]), counter=int(block[R.COUNTER]),
                G=np.array(block[R.HEADER:R.HEADER + n], dtype=np.float64))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _check(out, before, pred, target, rewards, cfg, T, n, K):
    """Every bar of the module docstring for one call; before: the block's state ahead of it.  -> the restated state behind it."""
    exact = R.exact_error(pred.numpy(), target.numpy())
    pos = exact > 0
    if pos.any():
        worst = float(np.max(np.abs(out["err"].astype(np.float64)[pos] - exact[pos]) / exact[pos]))
        print("T=%d n=%d K=%d: err rel %.3e (bar %.3e)" % (T, n, K, worst, R.err_bound(K)))
        assert worst <= R.err_bound(K)
    assert np.all(out["err"][~pos] == 0.0)
    ref = R.reference(None, None, None, before, gamma=cfg.gamma, normalize=bool(cfg.normalize), err=out["err"], **_sched(cfg))
    b = out["block"]
    got = _state_of(b, n)
    figs = (_rel(got["G"], ref["state"]["G"]), _rel(got["mean"], ref["state"]["mean"]), _rel(got["var"], ref["state"]["var"]))
    print("   G rel %.3e  mean rel %.3e  var rel %.3e (bar 1e-10)" % figs)
    assert max(figs) <= 1e-10
    assert got["count"] == ref["state"]["count"] == before["count"] + T * n and got["counter"] == before["counter"] + T
    # scale from the DEVICE's std, then bitwise
    std = float(b[R.STD])
    assert abs(std - np.sqrt(got["var"])) <= 2.0 ** -52 * std
    scale = R.scales(T, before["counter"], std, bool(cfg.normalize), **_sched(cfg))
    want_intr = out["err"] * scale[:, None]
    assert want_intr.dtype == np.float32 and np.array_equal(out["intrinsic"].view(np.uint32), want_intr.view(np.uint32))
    want_rew = rewards.numpy() + out["intrinsic"]
    assert want_rew.dtype == np.float32 and np.array_equal(out["rewards"].view(np.uint32), want_rew.view(np.uint32))
    # the logging slots: written, not accumulated
    assert b[R.ROWS] == T * n and b[R.WEIGHT_LAST] == R.weight(before["counter"] + T, **_sched(cfg))
    assert _rel(b[R.SUM_INTRINSIC], out["intrinsic"].astype(np.float64).sum()) <= 1e-10 or abs(b[R.SUM_INTRINSIC]) < 1e-300
    assert abs(b[R.SUM_REWARDS] - rewards.numpy().astype(np.float64).sum()) <= 1e-10 * np.abs(rewards.numpy()).astype(np.float64).sum()
    assert b[L.RND_TICKET_SCAN] == 0.0 and b[L.RND_TICKET_APPLY] == 0.0      # both arrival counters are zero between calls
    return got


# every extreme of each axis; n either side of the 64 rows / envs per workgroup of the first two launches (with T = 1 the rows are the
# envs) and of the 256 envs per work item of the third; K with and without 16-byte rows, odd, and the bound
SHAPES = [(1, 1, 1), (2, 15, 3), (5, 16, 12), (1, 17, 16), (1, 63, 12), (1, 64, 33), (2, 65, 33), (5, 65, 64), (2, 255, 1), (1, 256, 16), (5, 257, 64),
          (1, 1025, 64), (5, 1025, 1), (2, 1025, 12),
          (8, 17, 4), (11, 65, 3), (19, 257, 12),      # T >= 8: the scan loads eight steps at a time, then a tail of T % 8
          (5, 4097, 3),            # 65 scan workgroups: the last arriver's lane 0 adds two partials
          (1025, 1, 1),            # 1025 apply items on 1024 workgroups: one workgroup walks two items
          (300, 1025, 2),          # 1500 apply items, 17 scan workgroups, 4805 error tiles
          (1, 65536 * 64 + 65, 1)]      # 65538 error tiles on 65536 workgroups, 65538 scan workgroups, 16385 apply items


@pytest.mark.parametrize("T,n,K", SHAPES)
def test_against_the_restatement(T, n, K):
    pred, target, rewards = _inputs(T, n, K, 1000 * T + n + K)
    block = L.rnd_block(n, DEV)
    assert block.numel() == R.block_doubles(n)
    cfg = _cfg(gamma=0.97, w0=0.75)
    out = _check(_run(T, n, K, pred, target, rewards, cfg, block), R.fresh_state(n), pred, target, rewards, cfg, T, n, K)
    assert out["counter"] == T


def test_two_calls_carry_the_state():
    T, n, K = 5, 257, 12
    block = L.rnd_block(n, DEV)
    cfg = _cfg(gamma=0.9, schedule=R.LINEAR, w0=2.0, final_value=0.5, initial_step=3, final_step=8)      # the line spans both calls
    state = R.fresh_state(n)
    for call in range(2):
        pred, target, rewards = _inputs(T, n, K, 50 + call)
        state = _check(_run(T, n, K, pred, target, rewards, cfg, block), state, pred, target, rewards, cfg, T, n, K)
    assert state["counter"] == 2 * T and state["count"] == 2 * T * n
    assert np.all(state["G"] > 0)


def test_zero_variance_takes_the_else_branch():
    """var planted at 0 with count > 0 and all-zero errors: the merged var stays 0, std = 0, and scale is the weight itself."""
    T, n, K = 2, 17, 4
    block = L.rnd_block(n, DEV)
    block[R.VAR] = 0.0
    block[R.COUNT] = 100.0
    x = torch.randn(T, n, K)
    rewards = torch.randn(T, n)
    out = _run(T, n, K, x, x.clone(), rewards, _cfg(w0=3.0), block)
    assert out["block"][R.STD] == 0.0 and out["block"][R.VAR] == 0.0 and out["block"][R.WEIGHT_LAST] == 3.0
    assert np.all(out["err"] == 0.0) and np.all(out["intrinsic"] == 0.0) and np.all(np.isfinite(out["rewards"]))


def test_equal_embeddings_leave_the_rewards_alone():
    T, n, K = 5, 65, 16
    x = torch.randn(T, n, K)
    rewards = torch.randn(T, n)
    rewards[0, 0] = 0.0
    out = _run(T, n, K, x, x.clone(), rewards, _cfg(w0=1.0), L.rnd_block(n, DEV))
    assert not out["intrinsic"].any() and not np.signbit(out["intrinsic"]).any()
    assert np.array_equal(out["rewards"].view(np.uint32), rewards.numpy().view(np.uint32))


@pytest.mark.parametrize("cfg", [dict(schedule=R.CONSTANT, w0=0.5), dict(schedule=R.STEP, w0=0.5, final_value=0.125, final_step=103),
                                 dict(schedule=R.LINEAR, w0=1.0, final_value=0.25, initial_step=101, final_step=104),
                                 dict(schedule=R.LINEAR, w0=0.0, final_value=2.0, initial_step=98, final_step=103)],
                         ids=["constant", "step", "linear", "linear-rising"])
@pytest.mark.parametrize("normalize", [True, False])
def test_schedules_switch_inside_the_rollout(cfg, normalize):
    """The counter planted at 100, T = 5: rows use c = 101 .. 105, so every edge of every schedule falls inside the rollout."""
    T, n, K = 5, 33, 3
    block = L.rnd_block(n, DEV)
    block[R.COUNTER] = 100.0
    pred, target, rewards = _inputs(T, n, K, 9)
    c = _cfg(normalize=normalize, **cfg)
    before = dict(R.fresh_state(n), counter=100)
    out = _run(T, n, K, pred, target, rewards, c, block)
    _check(out, before, pred, target, rewards, c, T, n, K)
    w = [R.weight(100 + t + 1, **_sched(c)) for t in range(T)]
    if cfg["schedule"] != R.CONSTANT:
        assert len(set(w)) > 1      # the switch really is inside
    if not normalize:
        np.testing.assert_array_equal(out["intrinsic"], out["err"] * np.array(w, dtype=np.float32)[:, None])


def test_same_inputs_same_bits():
    T, n, K = 5, 1025, 12
    pred, target, rewards = _inputs(T, n, K, 4)
    outs = []
    for rep in range(2):
        block = L.rnd_block(n, DEV)
        for call in range(2):
            o = _run(T, n, K, pred, target, rewards, _cfg(gamma=0.95), block)
        outs.append(o)
    for k in ("err", "intrinsic", "rewards"):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), k
    assert np.array_equal(outs[0]["block"].view(np.uint64), outs[1]["block"].view(np.uint64))


@pytest.mark.parametrize("T,n,K,skew", [(2, 17, 3, 0), (5, 257, 12, 0), (1, 65, 16, 4), (3, 1025, 5, 0)])
def test_guard_bands(T, n, K, skew):
    """Every pointer carved at exactly the stated size between guard bands (the block: HGYM_RND_BLOCK_DOUBLES(n) doubles, written by
    hgym_rnd_block_init); bands clean after every call; outputs equal to the plain twin's bits.  skew = 4: embeddings that are not
    16-byte aligned take the scalar loads."""
    pred, target, rewards = _inputs(T, n, K, 77)
    cfg = _cfg(gamma=0.9, schedule=R.STEP, w0=1.0, final_value=0.5, final_step=T)

    def case(A):
        p, q = A.place(pred.to(DEV), skew=skew), A.place(target.to(DEV), skew=skew)
        r = A.place(rewards.to(DEV))
        err, intr = A.carve((T, n), F32), A.carve((T, n), F32)
        block = A.carve(R.block_doubles(n), F64)
        L.check(L.lib.hgym_rnd_block_init(n, L.f64ptr(block), _s()), "hgym_rnd_block_init")
        torch.cuda.synchronize()
        A.verify("hgym_rnd_block_init")
        assert float(block[R.VAR]) == 1.0 and float(block.sum()) == 1.0      # every double written: no guard byte (NaN) is left inside
        for call in range(2):
            L.check(L.lib.hgym_rnd_rewards(T, n, K, L.fptr(p), L.fptr(q), L.fptr(r), L.fptr(err), L.fptr(intr), C.byref(cfg), L.f64ptr(block), _s()),
                    "hgym_rnd_rewards")
            torch.cuda.synchronize()
            A.verify("hgym_rnd_rewards call %d" % call)
        return dict(err=err, intrinsic=intr, rewards=r, block=block)

    twin = case(G.Plain(DEV))
    arena = G.Arena(DEV, G.arena_bytes(*([4 * T * n * K] * 2 + [4 * T * n] * 3 + [8 * R.block_doubles(n)])))
    got = case(arena)
    for k in twin:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(twin[k].view(torch.uint8), got[k].view(torch.uint8)), k


def test_bad_arguments_write_nothing():
    T, n, K = 2, 17, 4
    pred, target, rewards = (t.to(DEV) for t in _inputs(T, n, K, 1))
    err, intr = torch.full((T, n), 7.0, device=DEV), torch.full((T, n), 7.0, device=DEV)
    block = L.rnd_block(n, DEV)
    keep = [t.clone() for t in (rewards, err, intr, block)]
    call = lambda T_, n_, K_, c, blk=block, p=pred: L.lib.hgym_rnd_rewards(T_, n_, K_, L.fptr(p), L.fptr(target), L.fptr(rewards), L.fptr(err), L.fptr(intr),
                                                                         None if c is None else C.byref(c), L.f64ptr(blk), _s())
    bad = [(0, n, K, _cfg()), (T, 0, K, _cfg()), (T, n, 0, _cfg()), (T, n, R.MAX_OUTPUTS + 1, _cfg()), (T, n, K, _cfg(gamma=1.0)), (T, n, K, _cfg(gamma=-0.5)),
           (T, n, K, _cfg(w0=-1.0)), (T, n, K, _cfg(w0=float("nan"))), (T, n, K, _cfg(w0=float("inf"))), (T, n, K, _cfg(schedule=3)),
           (T, n, K, _cfg(schedule=R.STEP, final_value=-1.0, final_step=3)), (T, n, K, _cfg(schedule=R.LINEAR, initial_step=5, final_step=5)),
           (T, n, K, _cfg(schedule=R.LINEAR, initial_step=6, final_step=5)), (T, n, K, None)]
    for args in bad:
        assert call(*args) == -1, args
    assert call(T, n, K, _cfg(), None) == -1 and call(T, n, K, _cfg(), block, None) == -1
    torch.cuda.synchronize()
    for t, k in zip((rewards, err, intr, block), keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    assert call(T, n, K, _cfg()) == 0      # and the same buffers are fine with a good configuration
    torch.cuda.synchronize()
    assert float(block[R.COUNTER]) == T
