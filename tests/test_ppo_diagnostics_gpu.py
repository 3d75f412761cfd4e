"""-m gpu: the diagnostics pass behind an update (hgym_ppo_diag_reduce, hgym_ppo_diagnostics, PPO.diagnostics, runner.diag_interval).

The reference of every number is a float64 restatement written here (`_stats64`, `_forward64`): the per-row forms of the loss
(ppo.py:128-166) on the same fp32 inputs.  Bars: the three counts exactly -- the inputs are asserted to keep every row at least 1e-4
(relative) away from a threshold, two orders above anything fp32 can move a row by, and no row is ever excluded; max / min ratio and
every fp64 sum to 1e-5 relative (the project's fp32 bar; the per-row terms are fp32), the sum of ratio - 1 - log ratio against 1e-5 of
sum |ratio - 1| because it cancels.  Everything else is torch.equal: the order of summation is fixed."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLIP = 0.2
HALF_LOG_2PI = 0.9189385332046727
TOL = 1e-5
DEV = "cuda"


def _L():
    from hgym import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ float64 restatement
def _stats64(cols, std, clip):
    """cols: (actions, mu_old, sigma_old, mu_new, logp_old, values_old, returns, advantages, values_new) fp32 CPU tensors; std (12,).
    -> (the 16 sums as float64 in HGYM_DIAG_* order, sum |ratio - 1|, the smallest relative distance of any row to a threshold)."""
    L = _L()
    a, mo, so, mn, lpo, vo, R, A, vn = [c.double() for c in cols]
    s = std.double()
    clip32 = float(np.float32(clip))
    lo, hi = float(np.float32(1.0) - np.float32(clip)), float(np.float32(1.0) + np.float32(clip))      # torch.clamp's fp32 bounds
    out = [0.0] * L.DIAG_SUMS
    out[L.DIAG_RATIO_MAX], out[L.DIAG_RATIO_MIN] = -math.inf, math.inf
    if a.shape[0] == 0:
        return out, 0.0, math.inf
    lp = (-(a - mn) ** 2 / (2.0 * s * s) - s.log() - HALF_LOG_2PI).sum(1)
    dl = lp - lpo
    ratio = dl.exp()
    kl = ((s / so).log() + (so * so + (mo - mn) ** 2) / (2.0 * s * s) - 0.5).sum(1)
    sur = torch.maximum(-A * ratio, -A * ratio.clamp(lo, hi))
    ent = (0.5 + HALF_LOG_2PI + s.log()).sum()
    eo, en = R - vo, R - vn
    vals = {L.DIAG_COUNT: a.shape[0], L.DIAG_KL: kl.sum(), L.DIAG_APPROX_KL: (ratio - 1.0 - dl).sum(), L.DIAG_RATIO: ratio.sum(),
            L.DIAG_CLIPPED: ((ratio < lo) | (ratio > hi)).sum(), L.DIAG_RATIO_MAX: ratio.max(), L.DIAG_RATIO_MIN: ratio.min(),
            L.DIAG_SURROGATE: sur.sum(), L.DIAG_RET: R.sum(), L.DIAG_RET_SQ: (R * R).sum(), L.DIAG_ERR_OLD: eo.sum(),
            L.DIAG_ERR_OLD_SQ: (eo * eo).sum(), L.DIAG_ERR_NEW: en.sum(), L.DIAG_ERR_NEW_SQ: (en * en).sum(),
            L.DIAG_VALUE_CLIPPED: ((vn - vo).abs() > clip32).sum(), L.DIAG_ENTROPY: ent * a.shape[0]}
    for k, v in vals.items():
        out[k] = float(v)
    margin = min(float((ratio / lo - 1.0).abs().min()), float((ratio / hi - 1.0).abs().min()), float(((vn - vo).abs() / clip32 - 1.0).abs().min()))
    return out, float((ratio - 1.0).abs().sum()), margin


def _compare(got, want, abs_ratio, what):
    """-> the largest error seen, in units of the bar (relative error / 1e-5); asserts counts exactly, everything else to TOL."""
    L = _L()
    got = [float(x) for x in got[:L.DIAG_SUMS].tolist()]
    worst = 0.0
    for k in range(L.DIAG_SUMS):
        if k in (L.DIAG_COUNT, L.DIAG_CLIPPED, L.DIAG_VALUE_CLIPPED):
            assert got[k] == want[k], "%s: count slot %d is %r, float64 says %r" % (what, k, got[k], want[k])
            continue
        if math.isinf(want[k]):
            assert got[k] == want[k], (what, k, got[k], want[k])
            continue
        scale = abs_ratio if k == L.DIAG_APPROX_KL else abs(want[k])
        err = abs(got[k] - want[k]) / scale if scale > 0 else abs(got[k] - want[k])
        worst = max(worst, err)
        assert err <= TOL, "%s: slot %d is %.12g, float64 says %.12g (relative error %.3g > %g)" % (what, k, got[k], want[k], err, TOL)
    return worst


def _columns(M, seed, plant):
    """Nine fp32 CPU columns + std.  plant: overwrite the first rows so that ratio lands at (1 +- clip)(1 +- 1e-3), |V_new - V_old| at
    clip (1 +- 1e-3), and one ratio each at exp(+20) and exp(-20)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    std = torch.rand(12, generator=g) * 0.7 + 0.5
    mn = rn(M, 12) * 0.5
    mo = mn + rn(M, 12) * 0.1
    so = (std * (1.0 + 0.1 * (torch.rand(12, generator=g) - 0.5))).expand(M, 12).contiguous()
    a = mo + so * rn(M, 12)
    lp64 = (-(a.double() - mn.double()) ** 2 / (2.0 * std.double() ** 2) - std.double().log() - HALF_LOG_2PI).sum(1)
    lpo = (lp64 + 0.15 * rn(M).double()).float()
    # (returns, value errors and advantages with a mean: a sum that cancels to nothing has no relative error to speak of)
    vo, R, A = rn(M), rn(M) * 1.5 + 0.8, rn(M) - 1.2
    vn = vo + 0.1 * rn(M)
    if plant:
        lo, hi = float(np.float32(1.0) - np.float32(CLIP)), float(np.float32(1.0) + np.float32(CLIP))
        targets = [lo * (1 - 1e-3), lo * (1 + 1e-3), hi * (1 - 1e-3), hi * (1 + 1e-3)]
        for i, t in enumerate(targets):
            lpo[i] = float(lp64[i] - math.log(t))
        lpo[4] = float(lp64[4] - 20.0)          # ratio exp(+20)
        lpo[5] = float(lp64[5] + 20.0)          # ratio exp(-20)
        A[4] = -abs(float(A[4])) - 0.5          # (its surrogate is then the unclipped, huge one)
        c32 = float(np.float32(CLIP))
        for i, (sg, f) in enumerate([(1, 1 - 1e-3), (1, 1 + 1e-3), (-1, 1 - 1e-3), (-1, 1 + 1e-3)]):
            vn[6 + i] = float(vo[6 + i]) + sg * c32 * f
    return [a, mo, so, mn, lpo, vo, R, A, vn], std


def _reduce(dcols, dstd, clip, m0, m1, total, finish, block):
    L = _L()
    ptrs = [L.fptr(t[m0:m1]) if m1 > m0 else None for t in dcols]
    return L.lib.hgym_ppo_diag_reduce(m1 - m0, *ptrs, L.fptr(dstd), clip, m0, total, finish, L.f64ptr(block),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _reset(total, block):
    L = _L()
    L.check(L.lib.hgym_ppo_diag_reset(total, L.f64ptr(block), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_ppo_diag_reset")


def _fresh_block(total):
    L = _L()
    b = torch.full((L.diag_block_doubles(total),), 7.25, dtype=torch.float64, device=DEV)      # reset must zero all of it
    _reset(total, b)
    return b


# ------------------------------------------------------------------------------------------------ the reduction alone
def test_reduction_on_planted_rows_matches_float64():
    """M = 777 in one call.  Largest error seen on MI355X: 1.11e-6 of the 1e-5 bar (printed below)."""
    L = _L()
    M = 777
    cols, std = _columns(M, 18, plant=True)
    want, abs_ratio, margin = _stats64(cols, std, CLIP)
    assert margin > 1e-4, "input condition: a row lies within 1e-4 of a threshold (%.3g); choose another seed" % margin
    assert 2 <= want[L.DIAG_CLIPPED] < M and 2 <= want[L.DIAG_VALUE_CLIPPED] < M
    assert want[L.DIAG_RATIO_MAX] > 4e8 and want[L.DIAG_RATIO_MIN] < 3e-9
    d = [c.to(DEV) for c in cols]
    block = _fresh_block(M)
    assert bool((block == 0).all())
    assert _reduce(d, std.to(DEV), CLIP, 0, M, M, 1, block) == 0, L.lib.hgym_last_error()
    torch.cuda.synchronize()
    worst = _compare(block.cpu(), want, abs_ratio, "M=777")
    print("diag reduce, M = 777 planted rows: largest error %.3g (bar %g)" % (worst, TOL))
    # the partials: 4 slots of 256 rows; their counts
    parts = block.cpu()[L.DIAG_SUMS:].view(-1, L.DIAG_SUMS)
    assert parts[:, L.DIAG_COUNT].tolist() == [256.0, 256.0, 256.0, 9.0]


@pytest.fixture(scope="module")
def ragged():
    cols, std = _columns(1000, 18, plant=False)
    return cols, std, [c.to(DEV) for c in cols], std.to(DEV)


@pytest.mark.parametrize("M", [0, 1, 63, 255, 256, 257, 1000])
def test_ragged_sizes(ragged, M):
    L = _L()
    cols, std, d, dstd = ragged
    want, abs_ratio, margin = _stats64([c[:M] for c in cols], std, CLIP)
    assert margin > 1e-4
    block = _fresh_block(M)
    assert _reduce(d, dstd, CLIP, 0, M, M, 1, block) == 0, L.lib.hgym_last_error()
    again = _fresh_block(M)
    assert _reduce(d, dstd, CLIP, 0, M, M, 1, again) == 0
    torch.cuda.synchronize()
    assert torch.equal(block, again)
    worst = _compare(block.cpu(), want, abs_ratio, "M=%d" % M)
    print("diag reduce, M = %d: largest error %.3g" % (M, worst))
    from hgym import diag_from_block
    r = diag_from_block(block.cpu(), CLIP)
    assert r["samples"] == M and (M > 0 or math.isnan(r["kl"]))


def test_piece_cuts_are_bit_identical_and_bad_cuts_refused(ragged):
    L = _L()
    cols, std, d, dstd = ragged
    M = 1000
    blocks = []
    for cuts in ([1000], [256, 256, 488], [768, 232]):
        b = _fresh_block(M)
        m0 = 0
        for i, n in enumerate(cuts):
            assert _reduce(d, dstd, CLIP, m0, m0 + n, M, 1 if i == len(cuts) - 1 else 0, b) == 0, L.lib.hgym_last_error()
            m0 += n
        blocks.append(b)
    torch.cuda.synchronize()
    assert torch.equal(blocks[0], blocks[1]) and torch.equal(blocks[0], blocks[2])
    assert float(blocks[0][L.DIAG_COUNT]) == 1000.0
    # refused, the block untouched: a non-final call that is no multiple of 256, a start that is none, rows beyond the block
    b = _fresh_block(M)
    b[:] = torch.arange(b.numel(), dtype=torch.float64, device=DEV)
    keep = b.clone()
    assert _reduce(d, dstd, CLIP, 0, 200, M, 0, b) == -1 and b"256" in L.lib.hgym_last_error()
    assert _reduce(d, dstd, CLIP, 100, 356, M, 1, b) == -1
    assert _reduce(d, dstd, CLIP, 768, 1000, 900, 1, b) == -1
    assert _reduce(d, dstd, CLIP, 0, 256, M, 2, b) == -1
    torch.cuda.synchronize()
    assert torch.equal(b, keep)


# ------------------------------------------------------------------------------------------------ the whole pass
def _net(no, npv, actor_hidden, critic_hidden, precision, max_batch, activation, seed):
    from hgym import NetBuffers, make_net_config
    net = NetBuffers(make_net_config(no, npv, 12, actor_hidden, critic_hidden, precision, max_batch, activation=activation), DEV)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.views.items():
        if k == "std":
            sd[k] = torch.rand(v.shape, generator=g) * 0.6 + 0.6
        elif k.endswith("weight"):
            sd[k] = torch.randn(v.shape, generator=g) / math.sqrt(v.shape[1])
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    net.load_state_dict(sd)
    return net, sd, g


def _forward64(sd, name, x, act):
    n = len([k for k in sd if k.startswith(name + ".") and k.endswith("weight")])
    h = x.double()
    for l in range(n):
        h = h @ sd["%s.%d.weight" % (name, 2 * l)].double().t() + sd["%s.%d.bias" % (name, 2 * l)].double()
        if l < n - 1:
            h = torch.where(h > 0, h, torch.expm1(h)) if act == "elu" else torch.tanh(h)
    return h


def _rows(M, no, npv, sd, g, act):
    """Stored rows whose old policy lies near the net's: (obs, priv, actions, values, advantages, returns, logp, mu, sigma) fp32 CPU."""
    rn = lambda *s: torch.randn(*s, generator=g)
    obs, priv = rn(M, no), rn(M, npv)
    mu64, v64 = _forward64(sd, "actor", obs, act), _forward64(sd, "critic", priv, act).squeeze(1)
    mo = (mu64 + 0.05 * rn(M, 12).double()).float()
    so = (sd["std"] * 1.05).expand(M, 12).contiguous()
    a = mo + so * rn(M, 12)
    lpo = (-(a.double() - mo.double()) ** 2 / (2.0 * so.double() ** 2) - so.double().log() - HALF_LOG_2PI).sum(1).float()
    vo = (v64 - 0.1 + 0.1 * rn(M).double()).float()
    R = (v64 + 0.4 + 0.5 * rn(M).double()).float()          # (sums with a mean, as in _columns)
    return [obs, priv, a, vo, rn(M) - 1.2, R, lpo, mo, so]


PASS_CASES = {
    "f32-elu": (47, 73, [64, 32], [64, 32], "f32", 256, 600, "elu"),
    "f32-tanh": (47, 73, [64, 32], [64, 32], "f32", 256, 600, "tanh"),
    "bf16-layers": (47, 73, [64, 32], [64, 32], "bf16", 256, 600, "elu"),
    "bf16-fused-xbotl": (705, 219, [512, 256, 128], [768, 256, 128], "bf16", 512, 512, "elu"),
}


@pytest.mark.parametrize("case", list(PASS_CASES))
def test_whole_pass_equals_forwards_plus_reduction(case):
    import torch.nn as nn
    from hgym import make_ppo_config
    L = _L()
    no, npv, ah, ch, precision, max_batch, M, act = PASS_CASES[case]
    net, sd, g = _net(no, npv, ah, ch, precision, max_batch, nn.Tanh() if act == "tanh" else None, 44)
    assert (net.shadow_ld(0) > 0) == (case == "bf16-fused-xbotl")        # the fused forward is exercised there, and only there
    rows = _rows(M, no, npv, sd, g, act)
    d = [t.to(DEV) for t in rows]
    ppo = make_ppo_config(clip_param=CLIP)
    opt_before, grads_before = net.opt_state.clone(), net.grads_ext.clone()
    block = torch.full((L.diag_block_doubles(M),), 3.5, dtype=torch.float64, device=DEV)
    net.ppo_diagnostics(ppo, d, block)
    again = torch.full_like(block, -1.0)
    net.ppo_diagnostics(ppo, d, again)
    # the same pieces by hand
    piece = max_batch if M <= max_batch else max_batch // 256 * 256
    manual = _fresh_block(M)
    obs, priv, a, vo, A, R, lpo, mo, so = d
    mu_all, v_all = [], []
    for m0 in range(0, M, piece):
        m1 = min(m0 + piece, M)
        mu, v = net.forward(0, obs[m0:m1]), net.forward(1, priv[m0:m1]).view(-1)
        mu_all.append(mu), v_all.append(v)
        ptr = [L.fptr(t[m0:m1]) for t in (a, mo, so)] + [L.fptr(mu)] + [L.fptr(t[m0:m1]) for t in (lpo, vo, R, A)] + [L.fptr(v)]
        assert L.lib.hgym_ppo_diag_reduce(m1 - m0, *ptr, L.fptr(net.params), CLIP, m0, M, 1 if m1 == M else 0, L.f64ptr(manual),
                                          net.stream()) == 0, L.lib.hgym_last_error()
    torch.cuda.synchronize()
    assert torch.equal(block, manual) and torch.equal(block, again)
    assert torch.equal(net.opt_state, opt_before) and torch.equal(net.grads_ext, grads_before)
    assert float(block[L.DIAG_COUNT]) == M
    if precision == "f32":
        # (the restated forward stays float64: mu_new and V_new enter _stats64 as doubles)
        _, _, ra, rvo, rA, rR, rlpo, rmo, rso = rows
        cols = [ra, rmo, rso, _forward64(sd, "actor", rows[0], act), rlpo, rvo, rR, rA, _forward64(sd, "critic", rows[1], act).squeeze(1)]
        want, abs_ratio, margin = _stats64(cols, sd["std"], CLIP)
        assert margin > 1e-4, margin
        worst = _compare(block.cpu(), want, abs_ratio, case)
        print("whole pass %s: largest error %.3g (bar %g)" % (case, worst, TOL))


# ------------------------------------------------------------------------------------------------ PPO.diagnostics
def _small_alg(monkeypatch, N, T):
    from humanoid.algo import PPO
    from humanoid.algo.ppo.actor_critic import ActorCritic
    monkeypatch.setattr(PPO, "precision", "f32")
    torch.manual_seed(3)
    ac = ActorCritic(47, 73, 12, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    alg = PPO(ac, num_learning_epochs=1, num_mini_batches=1, clip_param=CLIP, device=DEV)
    alg.init_storage(N, T, [47], [73], [12])
    return alg


def test_identity_when_the_parameters_have_not_moved(monkeypatch):
    N, T = 64, 5
    alg = _small_alg(monkeypatch, N, T)
    st = alg.storage
    with pytest.raises(RuntimeError, match="no update"):
        alg.diagnostics()
    g = torch.Generator(device=DEV).manual_seed(8)
    st._obs_all.copy_(torch.randn(st._obs_all.shape, device=DEV, generator=g))
    st._priv_all.copy_(torch.randn(st._priv_all.shape, device=DEV, generator=g))
    for s in range(T):          # what a rollout leaves in the slot, from the same rows and the same parameters
        alg.net.act(st._obs_all[s], st._priv_all[s], seed=77, step_counter=alg._sample_step,
                    out=dict(actions=st.actions[s], mu=st.mu[s], sigma=st.sigma[s], logp=st.actions_log_prob[s].view(-1), values=st.values[s]))
        alg._sample_step += 1
    st.returns.copy_(torch.randn(st.returns.shape, device=DEV, generator=g))
    st.advantages.copy_(torch.randn(st.advantages.shape, device=DEV, generator=g))
    assert float(st.actions.std()) > 0.3
    st.step = T
    # stand-in for an update that changes no parameter: prepare, the update's clear() (slot 0 <- slot T), "an update has run"
    alg.diagnostics_prepare()
    st.clear()
    with pytest.raises(RuntimeError, match="no update"):
        alg.diagnostics()
    alg._diag_updated = True
    slot0 = st._obs_all[0].clone()
    d = alg.diagnostics()
    print("identity:", d)
    assert torch.equal(st._obs_all[0], slot0) and torch.equal(st._obs_all[0], st._obs_all[T])      # slot 0 is as clear() left it
    assert d["samples"] == N * T and d["clip_fraction"] == 0.0 and d["value_clip_fraction"] == 0.0
    assert abs(d["ratio_max"] - 1.0) <= 1e-5 and abs(d["ratio_min"] - 1.0) <= 1e-5
    assert abs(d["kl"]) < 1e-6 and abs(d["approx_kl"]) < 1e-6
    assert d["explained_variance"] == d["explained_variance_new"] and d["value_rmse"] == d["value_rmse_new"]
    # without the saved rows the pass is refused, not run on the rotated slot
    alg._diag_saved = False
    with pytest.raises(RuntimeError, match="diagnostics_prepare"):
        alg.diagnostics()


TASK = "humanoid_ppo"


def _cfgs(num_envs, seed):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    return args, env_cfg, train_cfg


def _runner(num_envs, seed, log_root=None, **runner_keys):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    PPO.precision = "bf16"
    args, env_cfg, train_cfg = _cfgs(num_envs, seed)
    for k, v in runner_keys.items():
        setattr(train_cfg.runner, k, v)
    if "num_mini_batches" in runner_keys:
        train_cfg.algorithm.num_mini_batches = runner_keys["num_mini_batches"]
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=copy.deepcopy(env_cfg))
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=log_root)
    return runner


def _one_iteration(diag):
    """64 envs, 8 steps, the reference's plain loop (act / step / process_env_step), one update -> (runner, dicts)."""
    r = _runner(64, 17, num_steps_per_env=8, num_mini_batches=2)
    env, alg = r.env, r.alg
    obs, priv = env.get_observations(), env.get_privileged_observations()
    with torch.inference_mode():
        for _ in range(8):
            a = alg.act(obs, priv)
            obs, priv, rew, dones, infos = env.step(a)
            alg.process_env_step(rew, dones, infos)
        alg.compute_returns(priv)
    if diag:
        alg.diagnostics_prepare()
    alg.update()
    out = [alg.diagnostics(), alg.diagnostics()] if diag else []
    st = alg.storage
    torch.cuda.synchronize()
    state = dict(params=alg.net.params.clone(), opt=alg.net.opt_state.clone(), adam_m=alg.net.adam_m.clone(), obs_all=st._obs_all.clone(),
                 priv_all=st._priv_all.clone(), actions=st.actions.clone(), logp=st.actions_log_prob.clone(), mu=st.mu.clone(),
                 sigma=st.sigma.clone(), values=st.values.clone(), returns=st.returns.clone(), advantages=st.advantages.clone(),
                 rewards=st.rewards.clone(), dones=st.dones.clone())
    with torch.inference_mode():        # the next rollout's first step
        a = alg.act(obs, priv)
        obs2, priv2, rew2, _, _ = env.step(a)
    torch.cuda.synchronize()
    state.update(next_actions=a.clone(), next_obs=obs2.clone(), next_priv=priv2.clone(), next_rew=rew2.clone())
    return r, out, state


def test_after_a_real_update_and_no_side_effects():
    ra, (d1, d2), sa = _one_iteration(True)
    print("after one update:", d1)
    assert d1 == d2
    assert d1["samples"] == 512 and all(math.isfinite(v) for v in d1.values())
    assert d1["kl"] > 0 and d1["ratio_min"] <= 1.0 <= d1["ratio_max"]
    assert 0.0 <= d1["clip_fraction"] <= 1.0 and d1["return_std"] > 0 and d1["entropy"] > 0
    with pytest.raises(RuntimeError, match="no update"):      # the next rollout has begun
        ra.alg.diagnostics()
    rb, _, sb = _one_iteration(False)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), "`%s` differs from the twin run that never asked for diagnostics" % k


PLANS = {
    "eager": dict(HGYM_GRAPH="0", HGYM_GRAPH_UPDATE="0"),
    "stepwise": dict(HGYM_FUSE_ROLLOUT="0"),
    "deferred": dict(HGYM_ROLLOUT_CRITIC="deferred"),
    "sync": dict(HGYM_ASYNC="0"),
    "default": dict(),
}


class _Writer:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))


@pytest.mark.parametrize("logging", [False, True], ids=["nolog", "log"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_runner_diag_interval(monkeypatch, tmp_path, plan, logging):
    from hgym import DIAG_KEYS
    for k in ("HGYM_GRAPH", "HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_ROLLOUT_CRITIC", "HGYM_ASYNC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    finals = {}
    for interval in (2, 0):
        r = _runner(64, 23, log_root=str(tmp_path / ("d%d" % interval)) if logging else None, diag_interval=interval, save_interval=1000)
        w = _Writer()
        if logging:
            r.writer = w
            os.makedirs(r.log_dir, exist_ok=True)
        r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
        graphs = (r._rollout_capture.graph, r._update_capture.graph)
        keys = (r.alg.update_graph_key(), r.env.rollout_graph_key())
        if interval:
            assert r.last_diag_iteration == 1 and r.last_diag["samples"] == 64 * r.num_steps_per_env
            first = dict(r.last_diag)
        else:
            assert r.last_diag is None
        r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
        r.wait_for_saves()
        torch.cuda.synchronize()
        if interval:
            assert r.last_diag_iteration == 3 and tuple(r.last_diag) == DIAG_KEYS and r.last_diag != first
            assert all(math.isfinite(v) for v in r.last_diag.values()) and r.last_diag["kl"] > 0
            if logging:
                tags = [(t, s) for t, _, s in w.scalars if t.startswith("Diag/")]
                assert tags == [("Diag/" + k, it) for it in (1, 3) for k in DIAG_KEYS]
        else:
            assert not [t for t, _, _ in w.scalars if t.startswith("Diag/")]
        # the pass ran outside the graphs: nothing was re-captured, no key moved
        assert (r._rollout_capture.graph, r._update_capture.graph) == graphs
        assert (r.alg.update_graph_key(), r.env.rollout_graph_key()) == keys
        if plan in ("default", "deferred"):
            assert graphs[0] is not None and (graphs[1] is not None)
        finals[interval] = (r.alg.net.params.clone(), r.alg.net.opt_state.clone(), r.alg.storage._obs_all[0].clone())
    for x, y in zip(finals[2], finals[0]):
        assert torch.equal(x, y), "a run with diag_interval = 2 is not the run with diag_interval = 0 (%s)" % plan
