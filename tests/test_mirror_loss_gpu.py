"""-m gpu: the mirror loss of left-right symmetry (HgymPPOConfig.mirror_coef, PPO.mirror_loss_coef) on the device,
against the float64 reference of tests/mirror_loss_common.py at update_options_common's shapes and bars.

  1. gradient and mirror_sums of every new instantiation (fused: activation x value loss x input form; both layer paths: activation; one
     case each with log std, the auxiliary head, observation normalisation);
  2. the term alone (advantages, entropy and value coefficients 0): the actor's gradient at the same bars, the rest exactly zero;
  3. off is off: coefficient 0 with the five pointers set changes no bit; on, the critic, d std and the four loss sums keep their bits;
  4. batch edges on the fused path with the term on; rows beyond B (a NaN-filled target tail) add nothing;
  5. every misuse is refused with HGYM_E_BADARG and the gradient buffer is left alone;
  6. PPO.update in its three modes; 7. twenty Adam steps on the term alone lower the asymmetry; 8. a runner, captured against eager.

Storage columns are [rows | mirrored rows] (update_options_common.mirror_columns); the index slice is drawn over both halves and holds a
row together with its own partner.  The coefficient is mirror_loss_common.COEF = 0.5 everywhere."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_report as BR
import mirror_loss_common as M
import update_options_common as U
import test_update_options_gpu as G
from hgym import _lib as L

pytestmark = pytest.mark.gpu

O = U.Options
FUSED = [O("bf16-fused", act, "scalar", vu, False, False, sh) for act in (None, U.TANH) for vu in (False, True) for sh in (False, True)]
LAYER = [O(p, act, "scalar", False, False, False, False) for p in ("f32-layer", "bf16-layer") for act in (None, U.TANH)]
EXTRA = [O("bf16-fused", None, "log", False, False, False, True), O("bf16-fused", None, "scalar", False, True, False, True),
         O("bf16-fused", None, "scalar", False, False, True, True)]
CASES = FUSED + LAYER + EXTRA
WORST = {}      # path -> (worst gradient error / bar, which), printed by the last case of test 1


def _tables(case):
    return (torch.tensor(case["spec"].act_src, dtype=torch.int32, device="cuda"), torch.tensor(case["spec"].act_sign, dtype=torch.float32, device="cuda"))


def _grad(net, opts, case, ppo, shadow, mirror=True, rows=128):
    """One hgym_ppo_grad (+ the unfold) on the case; -> (mirror_sums on the host, the target scratch).  The target holds `rows` rows, NaN
    behind the minibatch's: a kernel that read a row beyond B would carry the NaN into the gradient or the sum."""
    from hgym import make_batch
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    A = cols[2].shape[1]
    target = torch.full((rows * A,), float("nan"), device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    if mirror:
        kw.update(pair_idx=case["pair"].cuda(), mirror=_tables(case) + (target, sums))
    net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
    net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
    net.ppo_grad(ppo, make_batch(*cols, case["idx"].cuda(), **kw))
    if opts.norm:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    return sums.cpu(), target


def _hold(what, opts, errs, bar):
    print("\n%s" % what)
    for k, e in errs.items():
        print("    %-20s %.3e  (bar %.1e)%s" % (k, e, bar, "  <-- above" if not e <= bar else ""))
    worst = max(errs, key=lambda k: errs[k] if errs[k] == errs[k] else float("inf"))
    if opts.path != "f32-layer":
        BR.check("%s (worst tensor: %s)" % (what, worst), errs[worst], bar)
    assert errs[worst] <= bar, "%s: %s measured %.3e > bar %.1e" % (what, worst, errs[worst], bar)
    return worst, errs[worst]


# ---------------------------------------------------------------------------------------------- 1. every new instantiation
@pytest.mark.parametrize("opts", CASES, ids=[U.case_id(o) for o in CASES])
def test_gradient_and_sums_of_every_instantiation(opts):
    case = M.case_of(opts)
    ref = M.reference(case)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, mirror_coef=M.COEF)
    sums, target = _grad(net, opts, case, ppo, opts.shadow)
    assert torch.isfinite(net.grads_ext).all()
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    name, e = _hold("mirror loss, gradient %s vs float64 reference" % U.case_id(opts), opts, U.errors(opts, got, ref), U.bar_of(opts))
    if e / U.bar_of(opts) > WORST.get(opts.path, (0.0,))[0]:
        WORST[opts.path] = (e / U.bar_of(opts), e, name, U.case_id(opts))
    assert float(sums[1]) == 1.0
    mse_err = abs(float(sums[0]) - ref["mirror"]) / ref["mirror"]
    print("    mirror_sums MSE %.6e vs %.6e: rel %.3e (bar %.1e)" % (float(sums[0]), ref["mirror"], mse_err, U.SUM_TOL[opts.path]))
    assert mse_err <= U.SUM_TOL[opts.path]
    _hold("mirror loss, loss sums %s" % U.case_id(opts), opts, U.sum_errors(opts, G._sums(net), ref), U.SUM_TOL[opts.path])
    B, A = case["B"], case["cols"][2].shape[1]
    assert torch.isfinite(target[:B * A]).all() and torch.isnan(target[B * A:]).all()      # the pre-pass wrote the minibatch's rows, no more
    if opts.shadow:      # the bf16 shadow rows and the fp32 rows give the same bits
        ext = net.grads_ext.clone()
        s2, _ = _grad(net, opts, case, ppo, False)
        assert torch.equal(ext.view(torch.int32), net.grads_ext.view(torch.int32)) and float(s2[0]) == float(sums[0])
    if opts == CASES[-1]:
        for path, w in WORST.items():
            print("worst gradient error with the mirror loss, %s: %.3e (%.2f of the bar; %s of %s)" % ((path, w[1], w[0]) + w[2:]))


# ---------------------------------------------------------------------------------------------- 2. the term alone
ALONE = [O(p, None, "scalar", False, False, False, p == "bf16-fused") for p in U.PATHS]


def _alone(case):
    cols = list(case["cols"])
    cols[4] = torch.zeros_like(cols[4])      # advantages
    return dict(case, cols=cols, ppo=dict(case["ppo"], value_coef=0.0, entropy_coef=0.0))


@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_the_term_alone(opts):
    """Advantages 0, entropy coefficient 0, value coefficient 0: the actor's gradient is the mirror term's and nothing else's -- held at the
    path's bars, so a wrong factor cannot hide under the surrogate's gradient; the critic's gradient and d std are exactly zero."""
    case = _alone(M.case_of(opts))
    ref = M.reference(case)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, mirror_coef=M.COEF, value_loss_coef=0.0, entropy_coef=0.0)
    _grad(net, opts, case, ppo, opts.shadow)
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    actor = [k for k in got if k.startswith("actor.")]
    _hold("mirror term alone %s: actor gradient vs float64 reference" % U.case_id(opts), opts,
          U.errors(opts, got, ref, names=actor), U.bar_of(opts))
    for k, g in got.items():
        if k not in actor:
            assert bool((g == 0).all()), k
            assert bool((ref["grads"][k] == 0).all()), k
    assert all(float(got[k].abs().max()) > 0 for k in actor)


# ---------------------------------------------------------------------------------------------- 3. off is off
OFF = ALONE + [O("bf16-fused", U.TANH, "scalar", True, False, False, False)]


@pytest.mark.parametrize("opts", OFF, ids=[U.case_id(o) for o in OFF])
def test_off_is_off(opts):
    case = M.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    off = G._ppo(opts, case)
    assert off.mirror_coef == 0.0
    _grad(net, opts, case, off, opts.shadow, mirror=False)
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    sums, target = _grad(net, opts, case, off, opts.shadow, mirror=True)
    assert torch.equal(g0.view(torch.int32), net.grads_ext.view(torch.int32)) and torch.equal(o0.view(torch.int64), net.opt_state.view(torch.int64))
    assert float(sums[0]) == 0.0 and float(sums[1]) == 0.0 and torch.isnan(target).all()      # ignored: nothing written
    _grad(net, opts, case, G._ppo(opts, case, mirror_coef=M.COEF), opts.shadow)
    views, base = net.views, net.params.data_ptr()
    flat0, flat1 = g0[:net.P], net.grads_ext[:net.P]
    moved = 0
    for k, v in views.items():
        o = (v.data_ptr() - base) // 4
        a, b = flat0[o:o + v.numel()], flat1[o:o + v.numel()]
        if k.startswith("actor."):
            moved += int(not torch.equal(a, b))
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s moved with the mirror loss on" % k
    assert moved == len([k for k in views if k.startswith("actor.")])
    assert torch.equal(g0[net.P:net.P + 1].view(torch.int32), net.grads_ext[net.P:net.P + 1].view(torch.int32))      # the KL slot
    for slot in (L.OPT_KL_SUM, L.OPT_SURROGATE_SUM, L.OPT_VALUE_SUM, L.OPT_ENTROPY_SUM, L.OPT_KL_LAST, L.OPT_MINIBATCHES):
        assert float(o0[slot]) == float(net.opt_state[slot]), slot


# ---------------------------------------------------------------------------------------------- 4. batch edges
@pytest.mark.parametrize("B", [1, 63, 64, 65, 97])
def test_fused_batch_edges_with_the_term_on(B):
    opts = O("bf16-fused", None, "scalar", False, False, False, True)
    case = M.make_case(opts, seed=40 + B, B=B)
    ref = M.reference(case)
    net = G._net(opts)
    G._load(net, opts, case)
    sums, target = _grad(net, opts, case, G._ppo(opts, case, mirror_coef=M.COEF), True)
    assert torch.isfinite(net.grads_ext).all() and torch.isnan(target[B * 12:]).all() and torch.isfinite(target[:B * 12]).all()
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    _hold("mirror loss, fused path, B = %d" % B, opts, U.errors(opts, got, ref), U.bar_of(opts))
    assert abs(float(sums[0]) - ref["mirror"]) <= U.SUM_TOL[opts.path] * ref["mirror"] and float(sums[1]) == 1.0


# ---------------------------------------------------------------------------------------------- 5. misuse
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_misuse_is_refused(opts):
    from hgym import make_batch
    case = M.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    cols = [t.cuda().contiguous() for t in case["cols"]]
    A = cols[2].shape[1]
    target, sums = torch.zeros(128 * A + 4, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    idx, pair = case["idx"].cuda(), case["pair"].cuda()
    net.grads_ext.fill_(7.0)
    torch.cuda.synchronize()

    def rc(ppo, batch, fn="grad"):
        if fn == "grad":
            return int(L.lib.hgym_ppo_grad(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(batch), net.stream()))
        if fn == "part":
            return int(L.lib.hgym_ppo_grad_part(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(batch), 0, net.stream()))
        return int(L.lib.hgym_ppo_apply(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), net.stream()))
    good = lambda: make_batch(*cols, idx, pair_idx=pair, mirror=_tables(case) + (target, sums))
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        ppo = G._ppo(opts, case, mirror_coef=bad)
        for fn in ("grad", "part", "apply"):
            assert rc(ppo, good(), fn) == -1, (bad, fn)      # HGYM_E_BADARG
            assert b"mirror_coef" in L.lib.hgym_last_error()
    ppo = G._ppo(opts, case, mirror_coef=M.COEF)
    for field in ("pair_idx", "mirror_act_src", "mirror_act_sign", "mirror_target", "mirror_sums"):
        b = good()
        setattr(b, field, None)
        for fn in ("grad", "part"):
            assert rc(ppo, b, fn) == -1, (field, fn)
    b = good()
    b.mirror_target = C.cast(target.data_ptr() + 4, L.c_float_p)      # not 16-byte aligned
    assert rc(ppo, b) == -1 and b"16-byte" in L.lib.hgym_last_error()
    torch.cuda.synchronize()
    assert bool((net.grads_ext == 7.0).all()) and float(sums.sum()) == 0.0      # nothing was launched


# ---------------------------------------------------------------------------------------------- 6. PPO.update
T_UP, N_UP = G.T_SYM, G.N_SYM
UP_OPTS = O("bf16-fused", None, "scalar", False, False, False, True)


def _update_run(monkeypatch, coef, augmentation, seed=31):
    import hgym
    from humanoid.algo import PPO
    spec = G._spec()
    if coef is not None:
        monkeypatch.setattr(PPO, "mirror_loss_coef", coef)
    if augmentation is not None:
        monkeypatch.setattr(PPO, "symmetry_augmentation", augmentation)
    alg = U._alg(monkeypatch, "bf16", N_UP, T_UP, spec)
    U._fill_rollout(alg, seed)
    st, net = alg.storage, alg.net
    obs = st._obs_store[:T_UP].flatten(0, 1).clone().cpu()
    pair_log, params_log = [], []
    make_batch, ppo_grad = hgym.make_batch, net.ppo_grad

    def mb(*a, **k):
        pair_log.append(None if k.get("pair_idx") is None else k["pair_idx"].clone())
        return make_batch(*a, **k)

    def pg(cfg, batch):
        params_log.append({k: v.clone().cpu() for k, v in net.state_dict().items()})
        ppo_grad(cfg, batch)
    monkeypatch.setattr(hgym, "make_batch", mb)
    monkeypatch.setattr(net, "ppo_grad", pg)
    idx_log, _ = U._record_batches(monkeypatch, alg)
    alg.update()
    torch.cuda.synchronize()
    return alg, spec, obs, [i.cpu() for i in idx_log], [None if p is None else p.cpu() for p in pair_log], params_log


@pytest.mark.parametrize("augmentation", [True, False], ids=["augmentation+mirror", "mirror-alone"])
def test_update_with_the_mirror_loss(monkeypatch, augmentation):
    alg, spec, obs, idx_log, pair_log, params_log = _update_run(monkeypatch, M.COEF, augmentation)
    T, N = T_UP, N_UP
    st = alg.storage
    assert st.mirrored and alg._mirror_loss.coef == M.COEF and alg._augment is augmentation and alg._ppo_cfg.mirror_coef == M.COEF
    assert len(idx_log) == 2 == len(pair_log) == len(params_log)
    rows = (2 if augmentation else 1) * T * N
    full = torch.zeros((2 * T + 1) * N, obs.shape[1])
    full[:T * N] = obs
    full[(T + 1) * N:] = obs[:, torch.tensor(spec.obs_src)] * torch.tensor(spec.obs_sign, dtype=obs.dtype)
    seen, mses = [], []
    src, sign = torch.tensor(spec.act_src), torch.tensor(spec.act_sign, dtype=torch.float64)
    for idx, pair, params in zip(idx_log, pair_log, params_log):
        assert idx.numel() == rows // 2 == pair.numel()
        lo = idx < T * N
        assert torch.equal(pair, torch.where(lo, idx + (T + 1) * N, idx - (T + 1) * N))      # the right partner, through the bootstrap slot
        for t in (idx, pair):
            assert not bool(((t >= T * N) & (t < (T + 1) * N)).any()) and int(t.min()) >= 0 and int(t.max()) < (2 * T + 1) * N
        if not augmentation:
            assert bool(lo.all())      # only original rows are drawn, T N // num_mini_batches at a time
        else:
            assert bool(lo.any()) and bool((~lo).any())
        seen += idx.tolist()
        priv = torch.zeros(idx.numel(), 219)
        mu, _, _ = U.forward(UP_OPTS, params, None, full[idx], priv)
        mu_p, _, _ = U.forward(UP_OPTS, params, None, full[pair], priv)
        mses.append(float(((mu - sign * mu_p[:, src]) ** 2).mean()))
    assert len(set(seen)) == rows == len(seen)
    # the stored mirrored observations are the torch-mirrored ones, bit for bit (also when only the observations are mirrored)
    got = st._obs_store[T + 1:].flatten(0, 1).cpu()
    assert torch.equal(got.view(torch.int32), full[(T + 1) * N:].view(torch.int32))
    want = sum(mses) / len(mses)
    err = abs(alg.last_mirror_loss - want) / want
    print("last_mirror_loss %.6e vs float64 reference on the recorded batches %.6e: rel %.3e" % (alg.last_mirror_loss, want, err))
    assert err <= U.SUM_TOL["bf16-fused"] and mses[0] != mses[1]


def test_augmentation_alone_is_the_parents_update(monkeypatch):
    """Coefficient 0 set explicitly (and symmetry_augmentation = True) against a twin that leaves both attributes untouched: the same
    batches, no pair, no scratch, bit-identical parameters."""
    runs = []
    for coef, aug in ((0.0, True), (None, None)):
        alg, _, _, idx_log, pair_log, _ = _update_run(monkeypatch, coef, aug)
        assert alg._mirror_loss is None and alg._options == () and alg.last_mirror_loss is None and pair_log == [None, None]
        assert alg._augment and idx_log[0].numel() == T_UP * N_UP
        runs.append((alg.net.params.clone(), alg.net.adam_m.clone(), alg.net.adam_v.clone(), idx_log))
        monkeypatch.undo()
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))


def test_mirror_loss_without_tables_is_refused(monkeypatch):
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "mirror_loss_coef", 0.5)
    with pytest.raises(ValueError, match="MirrorSpec"):
        U._alg(monkeypatch, "bf16", N_UP, T_UP, None)


def test_augmentation_off_with_coefficient_zero_is_symmetry_off(monkeypatch):
    from humanoid.algo import PPO
    monkeypatch.setattr(PPO, "symmetry_augmentation", False)
    alg = U._alg(monkeypatch, "bf16", N_UP, T_UP, G._spec())
    assert alg._symmetry is None and not alg.storage.mirrored and not alg._augment
    assert int(alg.net.cfg.max_batch) == max(T_UP * N_UP // 2, N_UP)


# ---------------------------------------------------------------------------------------------- 7. the term lowers the asymmetry
def test_twenty_steps_on_the_term_alone_lower_the_asymmetry():
    opts = ALONE[0]
    case = _alone(M.case_of(opts))
    half, spec = case["half"], case["spec"]
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, mirror_coef=M.COEF, value_loss_coef=0.0, entropy_coef=0.0, adaptive=False)
    obs = case["cols"][0].cuda().contiguous()
    src, sign = torch.tensor(spec.act_src, device="cuda"), torch.tensor(spec.act_sign, dtype=torch.float64, device="cuda")

    def asym():      # (two calls: the net's max_batch is below the 2 * half stored rows)
        mu = net.forward(0, obs[:half].contiguous()).double().clone()
        mu_m = net.forward(0, obs[half:].contiguous()).double().clone()
        torch.cuda.synchronize()
        return float(((mu - sign * mu_m[:, src]) ** 2).mean())
    before = asym()
    ref = M.asymmetry(opts, case["params"], case["stats"], case["cols"][0][:half], case["cols"][0][half:], spec)
    assert abs(before - ref) <= 1e-2 * ref
    for _ in range(20):
        _grad(net, opts, case, ppo, True)
        net.ppo_apply(ppo)
    after = asym()
    print("asymmetry of the stored rows: %.6e -> %.6e after 20 Adam steps on the mirror term alone" % (before, after))
    assert after < before


# ---------------------------------------------------------------------------------------------- 8. the runner, captured against eager
N_RUN, T_RUN = G.N_RUN, 8


def _runner(monkeypatch, log_root, augmentation, seed=57):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    monkeypatch.setattr(PPO, "precision", "bf16")
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N_RUN), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    env_cfg.seed = train_cfg.seed = seed
    train_cfg.runner.num_steps_per_env = T_RUN
    train_cfg.algorithm.symmetry = augmentation
    train_cfg.algorithm.mirror_loss_coef = M.COEF
    env, _ = task_registry.make_env(name="humanoid_ppo", args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name="humanoid_ppo", args=args, train_cfg=train_cfg, log_root=str(log_root))
    alg = runner.alg
    assert alg.storage.mirrored and alg._mirror_loss.coef == M.COEF and alg._augment is augmentation and alg._ppo_cfg.mirror_coef == M.COEF
    return runner


@pytest.mark.parametrize("augmentation", [False, True], ids=["mirror-alone", "augmentation+mirror"])
def test_runner_captured_as_eager(monkeypatch, tmp_path, augmentation):
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(monkeypatch, tmp_path / ("u" + mode), augmentation)
        r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
        r.wait_for_saves()
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (mode == "1")
        alg, net = r.alg, r.alg.net
        opt = net.opt_state.clone()
        if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
            opt[L.OPT_GRAD_SQNORM] = 0.0
        assert alg.last_mirror_loss is not None and alg.last_mirror_loss > 0.0
        runs[mode] = dict(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), opt_state=opt,
                          mirror_sums=alg._mirror_loss.sums.clone(), last=torch.tensor([alg.last_mirror_loss], dtype=torch.float64))
        for k, t in runs[mode].items():
            assert torch.isfinite(t).all(), (mode, k)
        if mode == "0":
            key = alg.update_graph_key()
            alg._ppo_cfg.mirror_coef = 0.25
            assert alg.update_graph_key() != key      # another coefficient re-captures
        del r
    assert G._same(runs["1"], runs["0"]) == []
