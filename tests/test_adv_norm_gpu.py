"""-m gpu: PPO.advantage_normalization on the device.

  1. hgym_adv_normalize_minibatches bit for bit against the existing hgym_adv_normalize run segment by segment on gathered copies, at every
     segment length at which the kernel takes another path, and against a float64 restatement at the project's bar for normalised
     advantages (tests/test_gae_gpu.py: rtol 1e-4, atol 2e-5).  The inputs are multiples of 2^-6 in [-8, 8]: every fp64 sum and sum of
     squares of them is exact in any order, so the host's statistics are the kernel's, whatever its reduction order.
  2. "none": compute_returns leaves returns - values.
  3. update() under "minibatch" against a twin under "none" whose advantages column holds what 1.'s reference arithmetic gives for the
     recorded slices: the same gradients after every minibatch, the same parameters -- the update reads the column and nothing else changes.
  4. the runner: the captured update against the eager one, diagnostics behind it, rsl_rl's key through the train config.
  5. "batch", the default, never touches any of it."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from update_options_common import _alg, _fill_rollout, _record_batches, xbot_l_spec

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 777.0
RTOL, ATOL = 1e-4, 2e-5      # tests/test_gae_gpu.py's bar for normalised advantages


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grid(n, g):
    """n multiples of 2^-6 in [-8, 8] (fp32, on the host)."""
    return torch.randint(-512, 513, (n,), generator=g).float() / 64.0


def _reference(adv, idx, segments):
    """The issue's reference for a column `adv` (device, fp32) and the slices of idx: per segment a contiguous gathered copy, its three
    statistics formed on the host in float64, the existing hgym_adv_normalize on the copy.  -> [normalised copy per segment] (device)."""
    from hgym import _lib as L
    seg_len = idx.numel() // segments
    out = []
    for s in range(segments):
        copy_ = adv[idx[s * seg_len:(s + 1) * seg_len]].contiguous()
        a = copy_.double().cpu().numpy()
        stats = torch.tensor([a.sum(), (a * a).sum(), float(seg_len)], dtype=torch.float64, device=DEV)
        L.check(L.lib.hgym_adv_normalize(seg_len, L.fptr(copy_), L.f64ptr(stats), _stream()), "hgym_adv_normalize")
        out.append(copy_)
    torch.cuda.synchronize()
    return out


def _float64(adv, idx, segments):
    a = adv[idx].double().cpu().numpy().reshape(segments, -1)
    mean = a.mean(axis=1, keepdims=True)
    std = np.sqrt(((a - mean) ** 2).sum(axis=1, keepdims=True) / (a.shape[1] - 1))
    return ((a - mean) / (std + 1e-8)).reshape(-1)


def _check_case(adv, idx, segments, rows):
    """One call on (adv, idx): drawn rows against both references, every undrawn row the sentinel, a second call the same bits."""
    import hgym
    from hgym import _lib as L
    seg_len = idx.numel() // segments
    scratch = L.adv_mb_scratch(segments, seg_len, DEV)
    out = torch.full((rows,), SENTINEL, device=DEV)
    hgym.adv_normalize_minibatches(idx, adv, out, segments, scratch)
    again = torch.full((rows,), SENTINEL, device=DEV)
    hgym.adv_normalize_minibatches(idx, adv, again, segments, scratch)      # the same scratch, never zeroed again
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    for s in range(segments):
        assert int(scratch.view(torch.int64)[3 * s + 2]) == 0      # the arrival counters are left zero
    want = _reference(adv, idx, segments)
    for s in range(segments):
        got = out[idx[s * seg_len:(s + 1) * seg_len]]
        assert torch.equal(got.view(torch.int32), want[s].view(torch.int32)), (segments, seg_len, s)
    undrawn = torch.ones(rows, dtype=torch.bool, device=DEV)
    undrawn[idx] = False
    assert int(undrawn.sum()) == rows - idx.numel() and bool((out[undrawn] == SENTINEL).all())
    np.testing.assert_allclose(out[idx].double().cpu().numpy(), _float64(adv, idx, segments), rtol=RTOL, atol=ATOL)      # every value
    return out


def _chunk():
    from hgym import _lib as L
    return L.ADV_MB_CHUNK


SEG_LENS = (2, 3, 63, 64, 65, 255, 256, 257, "c-1", "c", "c+1", "2c+1", 4161)


@pytest.mark.parametrize("seg_len", SEG_LENS, ids=[str(s) for s in SEG_LENS])
def test_kernel_equals_the_existing_kernel_segment_by_segment(seg_len):
    c = _chunk()
    seg_len = {"c-1": c - 1, "c": c, "c+1": c + 1, "2c+1": 2 * c + 1}.get(seg_len, seg_len)
    g = torch.Generator().manual_seed(1000 + seg_len)
    for segments in (1, 2, 4, 7):
        count = segments * seg_len
        rows = count + 37      # more rows than entries: 37 are never drawn
        # one segment of each case is constant (the last; with one segment a second call on a constant column)
        for constant in ((False, True) if segments == 1 else (True,)):
            adv = _grid(rows, g)
            idx = torch.randperm(rows, generator=g)[:count].contiguous()
            if constant:
                adv[idx[count - seg_len:]] = float(_grid(1, g))
            out = _check_case(adv.to(DEV), idx.to(DEV), segments, rows)
            if constant:
                last = out[idx[count - seg_len:].to(DEV)]
                assert bool((last.view(torch.int32) == 0).all())      # exactly +0: no NaN, no -0


def test_kernel_on_the_mirrored_layout_leaves_the_bootstrap_slot_alone():
    """(2 T + 1) N rows as RolloutStorage.enable_mirror lays them out, T = 3, N = 43: the 2 T N drawn rows lie on both sides of slot T."""
    T, N = 3, 43
    g = torch.Generator().manual_seed(77)
    rows = (2 * T + 1) * N
    valid = torch.cat((torch.arange(T * N), torch.arange((T + 1) * N, rows)))
    idx = valid[torch.randperm(valid.numel(), generator=g)].contiguous()
    out = _check_case(_grid(rows, g).to(DEV), idx.to(DEV), 2, rows)
    assert bool((out[T * N:(T + 1) * N] == SENTINEL).all())


def test_kernel_with_more_work_items_than_workgroups():
    """65 539 segments of two entries: more (segment, chunk) work items than the launch has workgroups (65 536), so workgroups walk them
    with a stride.  The existing kernel would take a launch per segment; the reference here is its arithmetic restated on the host --
    float64 statistics (exact on these inputs), then the fp32 operations in numpy, IEEE like the device's -- plus the float64 bar."""
    import hgym
    from hgym import _lib as L
    segments, seg_len = 65536 + 3, 2
    g = torch.Generator().manual_seed(9)
    count = segments * seg_len
    rows = count + 5
    adv, idx = _grid(rows, g), torch.randperm(rows, generator=g)[:count].contiguous()
    adv[idx[-2:]] = 1.25      # the last segment constant
    out = torch.full((rows,), SENTINEL, device=DEV)
    adv_d, idx_d = adv.to(DEV), idx.to(DEV)
    hgym.adv_normalize_minibatches(idx_d, adv_d, out, segments, L.adv_mb_scratch(segments, seg_len, DEV))
    torch.cuda.synchronize()
    a32 = adv[idx].numpy().reshape(segments, seg_len)
    a = a32.astype(np.float64)
    s1, s2, n = a.sum(axis=1), (a * a).sum(axis=1), float(seg_len)
    mean = (s1 / n).astype(np.float32)
    denom = np.sqrt(np.maximum((s2 - s1 * s1 / n) / (n - 1.0), 0.0)).astype(np.float32) + np.float32(1e-8)
    want = (a32 - mean[:, None]) / denom[:, None]
    assert want.dtype == np.float32
    got = out[idx_d].cpu().numpy().reshape(segments, seg_len)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not got[-1].any() and not np.signbit(got[-1]).any()
    np.testing.assert_allclose(got.reshape(-1).astype(np.float64), _float64(adv_d, idx_d, segments), rtol=RTOL, atol=ATOL)
    undrawn = torch.ones(rows, dtype=torch.bool)
    undrawn[idx] = False
    assert bool((out.cpu()[undrawn] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- 2. "none"
def _filled(monkeypatch, mode, precision="f32", N=43, T=3, symmetry=None, epochs=2, seed=31):
    """The update harness's algorithm in `mode` with a rollout in its storage; the advantages are multiples of 2^-6 (see the module's
    docstring: the reference of test 1 then has the kernel's statistics to the bit)."""
    from humanoid.algo import PPO
    if mode is not None:
        monkeypatch.setattr(PPO, "advantage_normalization", mode)
    alg = _alg(monkeypatch, precision, N, T, symmetry, epochs=epochs)
    _fill_rollout(alg, seed)
    st = alg.storage
    g = torch.Generator().manual_seed(seed)
    st.advantages.copy_(_grid(T * N, g).view(T, N, 1))
    return alg


def _with_rewards(alg, seed):
    st = alg.storage
    g = torch.Generator(device=DEV).manual_seed(seed)
    st.rewards.copy_(torch.randn(st.rewards.shape, device=DEV, generator=g))
    st.dones.copy_((torch.rand(st.dones.shape, device=DEV, generator=g) < 0.1).to(torch.uint8))


def test_none_and_minibatch_leave_the_raw_advantages(monkeypatch):
    got = {}
    for mode in ("batch", "none", "minibatch"):
        alg = _filled(monkeypatch, mode, N=48, T=5)
        st = alg.storage
        _with_rewards(alg, 5)
        alg.compute_returns(st._priv_all[st.num_transitions_per_env])
        torch.cuda.synchronize()
        got[mode] = (st.returns.clone(), st.advantages.clone(), st.values.clone())
        monkeypatch.undo()
    for mode in ("none", "minibatch"):
        ret, adv, val = got[mode]
        assert torch.equal(ret, got["batch"][0])      # returns: what "batch" leaves, bit for bit
        assert torch.equal(adv, ret - val)
    # ... and "batch" did standardise them
    b = got["batch"][1].double()
    assert abs(float(b.mean())) < 1e-5 and abs(float(b.std()) - 1.0) < 1e-5
    assert not torch.equal(got["batch"][1], got["none"][1])


# ---------------------------------------------------------------------------------------------- 3. the update reads the column
def _update_ab(monkeypatch, precision, symmetry):
    N, T = 43, 3
    aug = 2 if symmetry is not None else 1
    batch, mb = aug * T * N, aug * T * N // 2

    # run A: "minibatch"
    a = _filled(monkeypatch, "minibatch", precision, N, T, symmetry)
    st = a.storage
    assert st.advantages_mb is not None and st.advantages_mb.numel() == (T * N if symmetry is None else (2 * T + 1) * N)
    raw = st.advantages.clone()
    idx_a, grad_a = _record_batches(monkeypatch, a)
    a.update()
    torch.cuda.synchronize()
    assert len(idx_a) == 4 and all(i.numel() == mb for i in idx_a)      # two epochs of two minibatches
    assert torch.equal(idx_a[0], idx_a[2]) and torch.equal(idx_a[1], idx_a[3])      # one permutation for every epoch
    assert torch.equal(st.advantages, raw)      # the raw column is only read
    drawn = torch.cat(idx_a[:2])
    column = (st.advantages if symmetry is None else st._col_store["advantages"]).view(-1).clone()
    rows = column.numel()
    undrawn = torch.ones(rows, dtype=torch.bool, device=DEV)
    undrawn[drawn] = False
    assert int(undrawn.sum()) == rows - 2 * mb == (batch - 2 * mb) + (N if symmetry is not None else 0)
    assert batch - 2 * mb == (1 if symmetry is None else 0)      # 129 rows, two minibatches of 64: one row undrawn (258 = 2 x 129: none)
    assert bool((st.advantages_mb[undrawn].view(torch.int32) == 0).all())      # undrawn rows (and the bootstrap slot) hold 0
    if symmetry is not None:
        assert int((drawn >= (T + 1) * N).sum()) > 0 and int((drawn < T * N).sum()) > 0      # the slices reach past slot T
    want = _reference(column, drawn, 2)      # test 1's reference arithmetic on run A's recorded slices
    for s in range(2):
        assert torch.equal(st.advantages_mb[idx_a[s]].view(torch.int32), want[s].view(torch.int32))
    params_a, grads_a = a.net.params.clone(), [g.clone() for g in grad_a]
    monkeypatch.undo()

    # run B: "none", the same seed, its advantages column pre-filled with the reference's values
    b = _filled(monkeypatch, "none", precision, N, T, symmetry)
    sb = b.storage
    assert sb.advantages_mb is None
    filled = torch.zeros(rows, device=DEV)
    for s in range(2):
        filled[idx_a[s]] = want[s]
    if symmetry is None:
        sb.advantages.view(-1).copy_(filled)
    else:      # update() begins with storage.mirror(), which copies the original half of the column over the mirrored one: fill behind it
        real_mirror = sb.mirror

        def mirror(*args, **kwargs):
            real_mirror(*args, **kwargs)
            sb._col_store["advantages"].view(-1).copy_(filled)
        monkeypatch.setattr(sb, "mirror", mirror)
    idx_b, grad_b = _record_batches(monkeypatch, b)
    b.update()
    torch.cuda.synchronize()
    assert len(idx_b) == 4 and all(torch.equal(x, y) for x, y in zip(idx_a, idx_b))      # the same permutation: same seed, same draw
    assert all(float(g.abs().max()) > 0 for g in grads_a)
    for k, (ga, gb) in enumerate(zip(grads_a, grad_b)):
        assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "gradient of minibatch %d" % k
    assert torch.equal(params_a.view(torch.int32), b.net.params.view(torch.int32))
    return want


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_update_reads_the_normalised_column_and_nothing_else_changes(monkeypatch, precision):
    _update_ab(monkeypatch, precision, None)


def test_update_with_symmetry_augmentation_normalises_over_originals_and_mirrors(monkeypatch):
    want = _update_ab(monkeypatch, "bf16", xbot_l_spec())
    assert want[0].numel() == 129      # a minibatch's statistics are over its 129 drawn rows, mirrored ones among them


# ---------------------------------------------------------------------------------------------- 4. the runner
N_RUN, T_RUN = 64, 8


def _runner(monkeypatch, seed, **algorithm_keys):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    monkeypatch.setattr(PPO, "precision", "bf16")
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N_RUN), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    env_cfg.seed = train_cfg.seed = seed
    train_cfg.runner.num_steps_per_env = T_RUN
    train_cfg.runner.diag_interval = 1
    train_cfg.algorithm.num_mini_batches = 2      # minibatches of 256 rows: the diagnostics pass walks the batch in pieces of 256 (hgym_ppo_diagnostics)
    for k, v in algorithm_keys.items():
        setattr(train_cfg.algorithm, k, v)
    env, _ = task_registry.make_env(name="humanoid_ppo", args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name="humanoid_ppo", args=args, train_cfg=train_cfg, log_root=None)
    return runner


@pytest.mark.parametrize("keys,mode", [(dict(normalize_advantage_per_mini_batch=True), "minibatch"), (dict(advantage_normalization="none"), "none")],
                         ids=["rsl_rl-key-minibatch", "none"])
def test_runner_captured_as_eager_with_diagnostics(monkeypatch, keys, mode):
    from hgym import _lib as L, DIAG_KEYS
    runs = {}
    for graph_update in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", graph_update)
        torch.manual_seed(1357)
        np.random.seed(1357)
        r = _runner(monkeypatch, 61, **keys)
        alg, st = r.alg, r.alg.storage
        assert alg._adv_mode == mode and (st.advantages_mb is not None) == (mode == "minibatch")
        r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (graph_update == "1")
        assert r.last_diag_iteration == 2 and tuple(r.last_diag) == DIAG_KEYS and r.last_diag["samples"] == N_RUN * T_RUN
        assert all(math.isfinite(v) for v in r.last_diag.values()), r.last_diag
        net = alg.net
        opt = net.opt_state.clone()
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        runs[graph_update] = dict(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), opt_state=opt,
                                  diag=torch.tensor(list(r.last_diag.values()), dtype=torch.float64))
        if mode == "minibatch":
            runs[graph_update]["advantages_mb"] = st.advantages_mb.clone()
            # the raw column was left alone by compute_returns: returns - values of the last rollout
            assert torch.equal(st.advantages, st.returns - st.values)
            # 512 rows in two minibatches, each of mean 0 and unbiased deviation 1: the column's mean is 0, its deviation sqrt(510 / 511)
            adv = st.advantages_mb.double()
            assert abs(float(adv.mean())) < 1e-3 and 0.9 < float(adv.std()) < 1.1
        for k, t in runs[graph_update].items():
            assert torch.isfinite(t).all(), (graph_update, k)
        if graph_update == "0":
            key = alg.update_graph_key()
            assert dict(key)["obs_norm"] is alg._obs_norm and dict(key)["adv_mode"] == mode
            keep, alg._adv_mode = alg._adv_mode, "batch"
            assert alg.update_graph_key() != key      # another mode re-captures
            alg._adv_mode = keep
        del r
    for k in runs["1"]:
        assert torch.equal(runs["1"][k], runs["0"][k]), "`%s`: the captured update is not the eager one" % k


# ---------------------------------------------------------------------------------------------- 5. the default
def test_batch_mode_is_the_default_and_touches_nothing_new(monkeypatch):
    import hgym
    calls = []
    real = hgym.adv_normalize_minibatches
    logs = {}
    for mode in (None, "batch"):      # the attribute left as the class has it / set
        alg = _filled(monkeypatch, mode)
        monkeypatch.setattr(hgym, "adv_normalize_minibatches", lambda *a, **k: (calls.append(1), real(*a, **k)))
        assert alg._adv_mode == "batch" and alg.storage.advantages_mb is None and alg.storage._adv_mb_scratch is None
        key = alg.update_graph_key()
        assert (dict(key)["adv_mode"], dict(key)["adv_scratch"]) == ("batch", None)
        idx_log, grad_log = _record_batches(monkeypatch, alg)
        alg.update()
        torch.cuda.synchronize()
        assert alg.storage.advantages_mb is None
        logs[mode] = ([i.clone() for i in idx_log], [g.clone() for g in grad_log], alg.net.params.clone())
        monkeypatch.undo()
    assert not calls
    assert len(logs[None][1]) == 4
    for x, y in zip(logs[None][0] + logs[None][1] + [logs[None][2]], logs["batch"][0] + logs["batch"][1] + [logs["batch"][2]]):
        assert torch.equal(x, y)


def test_unknown_mode_and_one_row_minibatches_are_refused(monkeypatch):
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "advantage_normalization", "per_minibatch")
    with pytest.raises(ValueError, match="advantage_normalization"):
        _alg(monkeypatch, "f32", 8, 2, None)
    monkeypatch.setattr(PPO, "advantage_normalization", "minibatch")
    with pytest.raises(ValueError, match="at least 2 rows"):
        _alg(monkeypatch, "f32", 1, 3, None)      # 3 rows, two minibatches of one
