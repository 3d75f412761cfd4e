"""-m gpu: hgym_gae / hgym_gae_bootstrap / hgym_adv_normalize at their edges, against float64 restatements of rollout_storage.py:122-136.

gae_kernel walks T in 64-step tiles from the end with a scalar carry (lanes past the last step act as the identity map), sums the
advantage statistics per workgroup and lets the last workgroup to arrive add the partials in a fixed order (i += 256 past 256 workgroups,
N > 4096); adv_normalize_kernel grid-strides past 2048 x 256 elements.  The cases put a lone valid lane in the last tile (T = 65, 129),
dones on a tile edge and in the last step, gamma = lambda = 1 over 2 400 steps, lambda = 0 and gamma = 0, and N past every workgroup
boundary of the statistics."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_report as BR

pytestmark = pytest.mark.gpu

COEFS = [(0.994, 0.9), (1.0, 1.0), (0.99, 0.0), (0.0, 0.9)]
DONES = ["none", "all", "tile_edge", "last", "random"]
# Per element: |kernel - float64| <= GAE_TOL * scale, scale = |R64| + D_t, D_t = sum_k (prod c) (|r_k| + nt gamma |V_k+1| + |V_k|): the
# magnitudes every fp32 rounding of the scan is relative to, which cancellation in A_t does not shrink.  Roundings on the way to one
# element: 3 forming delta_t, 6 Kogge-Stone levels, one per tile through the carry (38 at T = 2 400), 2 forming R and R - V, and
# (gamma*lambda) rounded once to fp32 (k * 2^-24 on c^k, summed: <= 1 / (1 - c) = 10 roundings at 0.8946); <= 50 x 2^-24 = 3.0e-6 at
# gamma = lambda = 1, T = 2 400 (worst measured: see the report).
GAE_TOL = 1e-5
# The statistics: fp64 additions of fp32 values (squares exact in fp64), at most ~70 of them deep (per-lane tile sums, wave / block trees,
# the last arriver's i += 256 loop and trees): |err| <= 70 x 2^-53 x sum|a| = 7.8e-15 x sum|a|.
STATS_TOL = 1e-13


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(T, N, dones, seed, big_mean=False):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(T, N, generator=g) * 0.3
    v = torch.randn(T, N, generator=g) * 2 + 3
    lv = torch.randn(N, generator=g) * 2 + 3
    if big_mean:                                   # gamma = 0, V = 0: A = r, mean / std ~ 1e3
        r = 1000.0 + torch.randn(T, N, generator=g)
        v.zero_()
        lv.zero_()
    d = torch.zeros(T, N, dtype=torch.uint8)
    if dones == "all":
        d.fill_(1)
    elif dones == "tile_edge":                     # t = 62, 63, 64 (env e: 62 + e % 3), plus 1 %
        e = torch.arange(N)
        t = 62 + e % 3
        d[t[t < T], e[t < T]] = 1
        d |= (torch.rand(T, N, generator=g) < 0.01).to(torch.uint8)
    elif dones == "last":
        d[T - 1] = 1
    elif dones == "random":
        d = (torch.rand(T, N, generator=g) < 0.03).to(torch.uint8)
    # time-outs for hgym_gae_bootstrap: on a done and without one
    to = ((torch.rand(T, N, generator=g) < 0.05) & (d != 0)) | (torch.rand(T, N, generator=g) < 0.02)
    return r, v, d, to.to(torch.uint8), lv


def _run(kind, T, N, r, v, d, to, lv, gamma, lam, stats=None):
    """One launch on device copies; returns (rewards column after the call, returns, raw advantages, stats) on the host."""
    from hgym import _lib as L
    dev = "cuda"
    rew, val, dn, tod, last = (x.to(dev).contiguous() for x in (r, v, d, to, lv))
    ret, adv = torch.full((T, N), float("nan"), device=dev), torch.full((T, N), float("nan"), device=dev)
    st = L.gae_stats(N, dev) if stats is None else stats
    if kind == "gae":
        L.check(L.lib.hgym_gae(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dn), L.fptr(last), gamma, lam, L.fptr(ret), L.fptr(adv),
                               L.f64ptr(st), _stream()), "hgym_gae")
    else:
        L.check(L.lib.hgym_gae_bootstrap(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dn), L.u8ptr(tod), L.fptr(last), gamma, lam, L.fptr(ret),
                                         L.fptr(adv), L.f64ptr(st), _stream()), "hgym_gae_bootstrap")
    torch.cuda.synchronize()
    return rew.cpu(), ret.cpu(), adv.cpu(), st[:4].cpu().clone()


def _boot_rewards(r, v, to, gamma):
    """ppo.py:107-108 in store_step_kernel's three fp32 roundings: r + gamma * (V * time_out)."""
    r, v, to = r.numpy(), v.numpy(), to.numpy().astype(np.float32)
    return torch.from_numpy(r + np.float32(gamma) * (v * to))


def _gae64(r, v, d, lv, gamma, lam):
    """rollout_storage.py:122-133 in float64 on the kernel's inputs (gamma, lambda as the fp32 values it receives): (A64, R64, scale)."""
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    r, v, d, lv = (x.double().numpy() for x in (r, v, d, lv))
    T, N = r.shape
    A, D = np.zeros(N), np.zeros(N)
    adv, scale = np.empty((T, N)), np.empty((T, N))
    for t in reversed(range(T)):
        nxt = lv if t == T - 1 else v[t + 1]
        nt = 1.0 - d[t]
        c = nt * g * l
        A = r[t] + nt * g * nxt - v[t] + c * A
        D = np.abs(r[t]) + nt * g * np.abs(nxt) + np.abs(v[t]) + c * D
        adv[t], scale[t] = A, D
    ret = adv + v
    return adv, ret, scale + np.abs(ret)


def _check_stats(stats, raw, T, N, what):
    a = raw.double().numpy().ravel()
    mag = float(np.abs(a).sum())
    e0 = abs(float(stats[0]) - float(a.sum())) / max(mag, 1e-300)
    e1 = abs(float(stats[1]) - float((a * a).sum())) / max(float((a * a).sum()), 1e-300)
    assert float(stats[2]) == float(T * N) and float(stats[3]) == 0.0, what
    return e0, e1


@pytest.mark.parametrize("T,N", [(2, 1), (63, 15), (65, 17), (127, 16), (128, 17), (129, 17), (2400, 17), (64, 4097), (65, 8192),
                                 (129, 16384)])
def test_gae_edges_vs_float64(T, N):
    """Returns and advantages of both kernels against the float64 recurrence for every (gamma, lambda) and done pattern; the column
    hgym_gae_bootstrap writes back is store_step's bootstrap bit for bit; statistics [0], [1] against float64 sums of the kernel's own
    raw advantages, [2] exact, [3] (the arrival counter) back to zero."""
    worst = {"ret": 0.0, "adv": 0.0, "s0": 0.0, "s1": 0.0}
    for ci, (gamma, lam) in enumerate(COEFS):
        for di, dones in enumerate(DONES):
            r, v, d, to, lv = _inputs(T, N, dones, seed=T * 7919 + N * 31 + ci * 5 + di)
            for kind in ("gae", "bootstrap"):
                rew = _boot_rewards(r, v, to, gamma) if kind == "bootstrap" else r
                col, ret, adv, stats = _run(kind, T, N, r, v, d, to, lv, gamma, lam)
                what = "%s T=%d N=%d gamma=%g lambda=%g dones=%s" % (kind, T, N, gamma, lam, dones)
                assert torch.equal(col, rew), what + ": rewards column"
                if kind == "bootstrap" and gamma != 0.0 and bool(to.any()):
                    assert not torch.equal(rew, r)
                A64, R64, scale = _gae64(rew, v, d.float(), lv, gamma, lam)
                er = float((np.abs(ret.double().numpy() - R64) / scale).max())
                ea = float((np.abs(adv.double().numpy() - A64) / scale).max())
                assert er <= GAE_TOL and ea <= GAE_TOL, "%s: returns %.2e, advantages %.2e (x scale)" % (what, er, ea)
                e0, e1 = _check_stats(stats, adv, T, N, what)
                assert e0 <= STATS_TOL and e1 <= STATS_TOL, "%s: stats %.2e %.2e" % (what, e0, e1)
                for k, e in (("ret", er), ("adv", ea), ("s0", e0), ("s1", e1)):
                    worst[k] = max(worst[k], e)
    BR.check("gae T=%d N=%d: returns vs float64, worst / scale" % (T, N), worst["ret"], GAE_TOL)
    BR.check("gae T=%d N=%d: advantages vs float64, worst / scale" % (T, N), worst["adv"], GAE_TOL)
    BR.check("gae T=%d N=%d: stats[0] vs float64 sum, / sum|a|" % (T, N), worst["s0"], STATS_TOL)
    BR.check("gae T=%d N=%d: stats[1] vs float64 sum of squares, relative" % (T, N), worst["s1"], STATS_TOL)


@pytest.mark.parametrize("N", [8192, 16384])
def test_statistics_bits_across_runs_and_kernels(N):
    """Past 256 workgroups (the last arriver's i += 256 loop): two runs of each kernel, and hgym_gae on store_step's bootstrapped rewards
    vs hgym_gae_bootstrap on the raw ones, give the same bits -- statistics, returns and advantages."""
    T = 129
    r, v, d, to, lv = _inputs(T, N, "random", seed=N)
    boot = _boot_rewards(r, v, to, 0.994)
    a = _run("gae", T, N, boot, v, d, to, lv, 0.994, 0.9)
    b = _run("gae", T, N, boot, v, d, to, lv, 0.994, 0.9)
    c = _run("bootstrap", T, N, r, v, d, to, lv, 0.994, 0.9)
    e = _run("bootstrap", T, N, r, v, d, to, lv, 0.994, 0.9)
    for x in (b, c, e):
        for i in range(4):
            assert torch.equal(x[i], a[i]), i


def test_stats_buffer_reused_without_zeroing():
    """What the runner does every iteration: one `stats` buffer across calls, never zeroed again -- five calls at N = 8 192 with
    different T, then smaller N in the same buffer; each gives the bits of a fresh buffer.  And a buffer whose partial slots hold
    garbage (NaN, huge values) gives the fresh result: the last arriver reads only what this call wrote."""
    from hgym import _lib as L
    N = 8192
    shared = L.gae_stats(N, "cuda")
    calls = [(65, N), (129, N), (60, N), (2, N), (128, N), (64, 4097), (3, 17)]
    for i, (T, n) in enumerate(calls):
        r, v, d, to, lv = _inputs(T, n, "random", seed=100 + i)
        kind = "gae" if i % 2 == 0 else "bootstrap"
        got = _run(kind, T, n, r, v, d, to, lv, 0.994, 0.9, stats=shared)
        want = _run(kind, T, n, r, v, d, to, lv, 0.994, 0.9)
        for k in range(4):
            assert torch.equal(got[k], want[k]), (T, n, k)
        assert float(shared[3]) == 0.0
    for T, n in ((129, 16384), (65, 17)):
        r, v, d, to, lv = _inputs(T, n, "random", seed=T + n)
        dirty = L.gae_stats(n, "cuda")
        junk = torch.randn(dirty.numel() - 4, device="cuda", dtype=torch.float64) * 1e300
        junk[::3] = float("nan")
        dirty[4:] = junk
        got = _run("gae", T, n, r, v, d, to, lv, 0.994, 0.9, stats=dirty)
        want = _run("gae", T, n, r, v, d, to, lv, 0.994, 0.9)
        for k in range(4):
            assert torch.equal(got[k], want[k]), (T, n, k)


def _normalize(raw, stats):
    from hgym import _lib as L
    adv = raw.cuda().contiguous()
    stats_d = stats.to(torch.float64).cuda()
    L.check(L.lib.hgym_adv_normalize(adv.numel(), L.fptr(adv), L.f64ptr(stats_d), _stream()), "hgym_adv_normalize")
    torch.cuda.synchronize()
    return adv.cpu()


@pytest.mark.parametrize("T,N,big_mean", [(60, 16384, False), (2, 1, False), (1, 2, False), (65, 8192, True), (129, 17, True)])
def test_adv_normalize_vs_float64(T, N, big_mean):
    """rollout_storage.py:136 -- (a - mean) / (std_unbiased + 1e-8) -- of the kernel's own raw advantages in float64 two-pass: at
    60 x 16 384 = 983 040 elements (past the 2 048 x 256 grid: every thread takes two), at two elements, and at mean / std ~ 1e3.
    Bound, per element: the fp32 mean is off by <= 2^-24 |mean|, which moves the result by 2^-24 |mean| / std; the subtraction, the fp32
    std (sqrt rounded, + 1e-8 rounded) and the division add <= 4 x 2^-24 |result|."""
    gamma, lam = (0.0, 0.9) if big_mean else (0.994, 0.9)
    r, v, d, to, lv = _inputs(T, N, "random", seed=T * N, big_mean=big_mean)
    _, _, raw, stats = _run("gae", T, N, r, v, d, to, lv, gamma, lam)
    got = _normalize(raw, stats)
    a = raw.double().numpy().ravel()
    mean = a.mean()
    std = np.sqrt(((a - mean) ** 2).sum() / (a.size - 1))
    want = (a - mean) / (std + 1e-8)
    u = 2.0 ** -24
    bound = u * abs(mean) / std + 5 * u * np.abs(want) + 1e-30
    err = np.abs(got.double().numpy().ravel() - want)
    ratio = float((err / bound).max())
    BR.check("adv_normalize T=%d N=%d mean/std=%.0f: worst err / derived bound" % (T, N, abs(mean) / std), ratio, 1.0)
    if big_mean:
        assert abs(mean) / std > 500
