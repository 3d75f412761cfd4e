"""-m gpu: the PPO update with its options COMBINED -- activation x noise parametrisation x value loss x auxiliary
head x observation normalisation x bf16 input shadows on the three update paths, and symmetry on top -- against the ONE float64
reference of tests/update_options_common.py (pinned on the host by tests/test_update_options.py).

  a. the gradient of every combination (128 cases) at the project's bars, the loss sums, shadow on == shadow off bit for bit;
  b. one optimiser step leaves every derived copy current: operand copies, effective biases, the sigma block (32 cases);
  c. the doubled (symmetry) update with each other option against the reference on columns mirrored with torch;
  d. with symmetry on the normaliser merges the original rows only;
  e. the runner with everything on: captured == eager, and an exact resume is the run."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import bf16_report as BR
import obs_norm_common as ON
import update_options_common as U
from oracle import ppo_oracle as P
from hgym import _lib as L

pytestmark = pytest.mark.gpu

LR = 1e-3
FWD_TOL, FWD_MAX_TOL, F32_FWD_TOL = 2e-3, 5e-3, 1e-5      # tests/test_activations_gpu.py
IDS = [U.case_id(o) for o in U.MATRIX]
# a case whose bar differs from the path's, under the rule of DESIGN.md section 23 (fp32 accumulation alone, evaluated on the CPU, above
# a quarter of the bar): {case id: (bar, CPU fp32 error, reason)}.  Empty: every case holds the project's bars.
RAISED = {}

_NETS = {}


def _net(opts):
    """One NetBuffers per (path, activation, std, aux, norm), back at its initial optimiser state."""
    from hgym import NetBuffers, make_net_config
    key = (opts.path, opts.activation is not None, opts.std, opts.aux, opts.norm)
    if key not in _NETS:
        sh = U.SHAPES[opts.path]
        no, npv, A, ah, ch = sh["net"]
        kw = dict(aux_hidden=sh["aux"][0], aux_out=sh["aux"][1], aux_target_offset=sh["aux"][2]) if opts.aux else {}
        cfg = make_net_config(no, npv, A, ah, ch, "f32" if opts.path == "f32-layer" else "bf16", 64 if opts.path == "f32-layer" else 128,
                              activation=opts.activation, fused_activation=opts.path == "bf16-fused", noise_std_type=opts.std, **kw)
        net = NetBuffers(cfg, "cuda", learning_rate=LR, obs_norm=(U.EPS, None) if opts.norm else None)
        assert (net.shadow_ld(0) > 0) == (opts.path == "bf16-fused"), (opts, net.shadow_ld(0))
        if opts.path == "bf16-layer":
            assert net.shadow_ld(0) == 0
        assert list(net.views) == U.names_of(opts)
        _NETS[key] = net
    net = _NETS[key]
    for t in (net.adam_m, net.adam_v, net.opt_state, net.grads_ext):
        t.zero_()
    net.opt_state[L.OPT_LR] = LR
    return net


def _load(net, opts, case):
    """The case's parameters, then its statistics (count and all), then hgym_net_sync_shadow: every derived copy from this state."""
    net.load_state_dict(case["params"])
    if opts.norm:
        net.load_norm_state(U.norm_state_of(case["stats"]))
        net.sync_shadow()
        assert float(net.norm_view("header")[2]) == U.PLANTED_COUNT
        m, s = U.derived_stats(case["stats"])[0]
        assert np.array_equal(net.norm_view("mean_f", 0).cpu().numpy(), m)
        assert (np.abs(net.norm_view("scale_f", 0).cpu().numpy().astype(np.float64) - s) <= 2.0 ** -23 * np.abs(s)).all()
    torch.cuda.synchronize()


def _ppo(opts, case, **kw):
    from hgym import make_ppo_config
    return make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"], clipped_value_loss=not opts.unclipped, **kw)


def _grad(net, opts, case, ppo, shadow):
    from hgym import make_batch
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
    net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
    net.ppo_grad(ppo, make_batch(*cols, case["idx"].cuda(), **kw))
    if opts.norm:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    return cols


def _hold(what, opts, errs, bar, report=True):
    """Print every tensor's figure, then hold the worst to the bar (one line of the bf16 report per bf16 case)."""
    print("\n%s" % what)
    for k, e in errs.items():
        print("    %-20s %.3e  (bar %.1e)%s" % (k, e, bar, "  <-- above" if not e <= bar else ""))
    worst = max(errs, key=lambda k: errs[k] if errs[k] == errs[k] else float("inf"))
    if opts.path != "f32-layer" and report:
        BR.check("%s (worst tensor: %s)" % (what, worst), errs[worst], bar)
    assert errs[worst] <= bar, "%s: %s measured %.3e > bar %.1e" % (what, worst, errs[worst], bar)


def _sums(net):
    o = net.opt_state.cpu()
    return dict(surrogate=o[L.OPT_SURROGATE_SUM], value=o[L.OPT_VALUE_SUM], entropy=o[L.OPT_ENTROPY_SUM], kl=o[L.OPT_KL_LAST],
                aux=o[L.OPT_AUX_SUM])


# ---------------------------------------------------------------------------------------------- a. the gradient
@pytest.mark.parametrize("opts", U.MATRIX, ids=IDS)
def test_gradient_of_every_combination(opts):
    """hgym_ppo_grad (+ hgym_net_norm_unfold_grad) of one minibatch per combination against the float64 reference, per parameter
    tensor: rel-L2 5e-3 on both bf16 paths, max-abs over max-abs reference 5e-5 on f32, the critic's last bias against ||d_val||;
    the loss sums of opt_state's named slots; on the fused path the gradient gathered from bf16 shadows has the bits of the one
    gathered from the fp32 rows."""
    case, ref = U.case_of(opts), U.reference_of(opts)
    net = _net(opts)
    _load(net, opts, case)
    ppo = _ppo(opts, case)
    _grad(net, opts, case, ppo, opts.shadow)
    assert torch.isfinite(net.grads_ext).all()
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    sums = _sums(net)
    ext = net.grads_ext.clone()
    bar = RAISED[U.case_id(opts)][0] if U.case_id(opts) in RAISED else U.bar_of(opts)
    _hold("gradient %s vs float64 reference" % U.case_id(opts), opts, U.errors(opts, got, ref), bar)
    _hold("loss sums %s" % U.case_id(opts), opts, U.sum_errors(opts, sums, ref), U.SUM_TOL[opts.path], report=False)
    if not opts.aux:
        assert float(sums["aux"]) == 0.0
    if opts.shadow:
        _grad(net, opts, case, ppo, False)
        assert torch.equal(ext.view(torch.int32), net.grads_ext.view(torch.int32)), "shadow rows and fp32 rows give different bits"


# ---------------------------------------------------------------------------------------------- b. the step
STEP_CASES = [o for o in U.MATRIX if o.path in ("bf16-fused", "f32-layer") and not o.unclipped and not o.shadow]


def _outputs(net, opts, obs, priv, z):
    out = dict(mu=net.forward(0, obs), v=net.forward(1, priv))
    if opts.aux:
        out["aux"] = net.forward(2, obs)
    act = net.act(obs, priv, z=z)
    out.update(act_mu=act["mu"], act_v=act["values"], sigma=act["sigma"], logp=act["logp"], actions=act["actions"])
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("opts", STEP_CASES, ids=[U.case_id(o) for o in STEP_CASES])
def test_step_leaves_every_derived_copy_current(opts):
    """hgym_ppo_grad, the unfold, hgym_ppo_apply -- then, WITHOUT hgym_net_sync_shadow, the three forwards and hgym_policy_act on fresh
    raw rows against the float64 reference forward on the parameters read back from the device: the operand copies (scaled under
    normalisation), the effective biases and the sigma block are those of the NEW parameters.  A hgym_net_sync_shadow afterwards changes
    no bit.  The step itself is tests/test_optimizer_step_gpu.py's float64 clip + Adam on the device's own gradient.
    logp: the launch forms it from its own mu, actions and sigma in fp32 on every path, so it is held to the fp32 bar against the
    float64 expression of the device's mu and actions under the REFERENCE's sigma (a stale sigma block shows here)."""
    import test_optimizer_step_gpu as OS
    case = U.case_of(opts)
    sh = U.SHAPES[opts.path]
    no, npv, A = sh["net"][:3]
    net = _net(opts)
    _load(net, opts, case)
    ppo = _ppo(opts, case, adaptive=False)
    before = OS._state(net)
    _grad(net, opts, case, ppo, False)
    G = net.grads.double().cpu().numpy()
    net.ppo_apply(ppo)
    torch.cuda.synchronize()
    after = OS._state(net)
    what = "step %s" % U.case_id(opts)
    worst, _ = OS._check_step(before, after, G, math.fsum(G * G), 1, LR, ppo, what)
    BR.check("%s: clip + Adam on the device's own gradient, worst err / derived bound" % what, worst, 1.0)
    base = net.params.data_ptr()
    for k, v in net.views.items():
        o = (v.data_ptr() - base) // 4
        assert (after[0][o:o + v.numel()] != before[0][o:o + v.numel()]).any(), "%s did not move" % k
    assert (after[0][:A] != before[0][:A]).all()
    # fresh raw rows
    M = 33
    g = torch.Generator().manual_seed(77)
    if opts.norm:
        from test_obs_norm_gpu import _raw_rows
        e32 = float(np.float32(U.EPS))
        obs, priv = (torch.from_numpy(_raw_rows(M, case["stats"]["mean"][k], case["stats"]["var"][k], e32, g)) for k in (0, 1))
    else:
        obs, priv = torch.randn(M, no, generator=g), torch.randn(M, npv, generator=g)
    z = torch.randn(M, A, generator=g)
    out = _outputs(net, opts, obs.cuda(), priv.cuda(), z.cuda())
    params = {k: v.cpu() for k, v in net.state_dict().items()}
    mu, v, y = U.forward(opts, params, case["stats"], obs, priv)
    errs = {}
    for name, got, want in (("forward(0)", out["mu"], mu), ("forward(1)", out["v"], v), ("act mu", out["act_mu"], mu), ("act values", out["act_v"], v)) + \
            ((("forward(2)", out["aux"], y),) if opts.aux else ()):
        d = got.cpu().double().reshape(want.shape) - want
        assert torch.isfinite(got).all(), name
        if opts.path == "f32-layer":
            errs[name + ", worst / scale"] = (float(d.abs().max() / want.abs().max()), F32_FWD_TOL)
        else:
            errs[name + ", rel-L2"] = (float(d.norm() / want.norm()), FWD_TOL)
            errs[name + ", worst / scale"] = (float(d.abs().max() / want.abs().max()), FWD_MAX_TOL)
    sigma = U.sigma_of(opts, params)
    lp = P.gaussian_log_prob(out["actions"].cpu().double(), out["act_mu"].cpu().double(), out["act_mu"].cpu().double() * 0 + sigma)
    errs["logp, worst / scale"] = (float((out["logp"].cpu().double() - lp).abs().max() / lp.abs().max()), F32_FWD_TOL)
    print("\n%s" % what)
    for k, (e, b) in errs.items():
        print("    %-28s %.3e  (bar %.1e)%s" % (k, e, b, "  <-- above" if not e <= b else ""))
    for k, (e, b) in errs.items():
        if opts.path == "f32-layer":
            assert e <= b, (what, k, e, b)
        else:
            BR.check("%s: %s" % (what, k), e, b)
    # sigma: the parameter itself, or expf of it
    p_std = params[list(params)[0]]
    assert torch.equal(out["sigma"].cpu(), out["sigma"][0].cpu().expand(M, A))
    if opts.std == "scalar":
        assert torch.equal(out["sigma"][0].cpu().view(torch.int32), p_std.view(torch.int32))
    else:
        want = np.exp(p_std.numpy().astype(np.float64)).astype(np.float32)
        ulps = np.abs(out["sigma"][0].cpu().numpy().astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        assert float(ulps.max()) <= 2.0, ulps
        assert not torch.equal(out["sigma"][0].cpu(), p_std)
    net.sync_shadow()
    again = _outputs(net, opts, obs.cuda(), priv.cuda(), z.cuda())
    for k in out:
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), "%s changed under hgym_net_sync_shadow" % k


# ---------------------------------------------------------------------------------------------- c., d. symmetry
OTHERS = ("log", "norm", "unclipped", "aux", "tanh-fused", "all")
T_SYM, N_SYM = 4, 64


def _spec():
    from humanoid.envs import task_registry      # noqa: F401
    from humanoid.utils import task_registry as reg
    from humanoid.utils.symmetry import xbot_l_mirror
    return xbot_l_mirror(reg.get_cfgs("humanoid_ppo")[0])


def _sym_opts(other, precision):
    on = lambda name: other in (name, "all")
    return U.Options("f32-layer" if precision == "f32" else "bf16-fused", U.TANH if on("tanh-fused") else None, "log" if on("log") else "scalar",
                     on("unclipped"), on("aux"), on("norm"), precision == "bf16")


def _alg_with(monkeypatch, opts, precision, symmetry, T=T_SYM, N=N_SYM):
    """tests/test_symmetry_gpu.py's _alg with the options handed to ActorCritic and PPO; sigma away from 1; statistics planted."""
    import sys
    from humanoid.algo import PPO
    from humanoid.algo.ppo.actor_critic import ActorCritic as AC
    ACM, init = sys.modules[AC.__module__], PPO.__init__
    kw = dict(noise_std_type=opts.std, empirical_normalization=opts.norm, normalization_eps=U.EPS)
    if opts.activation is not None:
        kw.update(activation=opts.activation, fused_activation=True)
    if opts.aux:
        kw.update(denoiser_hidden_dims=[512, 256, 128] if precision == "bf16" else [64, 32], denoiser_targets=73)
    monkeypatch.setattr(ACM, "ActorCritic", lambda *a, **k: AC(*a, **dict(k, **kw)))
    monkeypatch.setattr(PPO, "__init__", lambda self, *a, **k: init(self, *a, **dict(k, use_clipped_value_loss=not opts.unclipped,
                                                                                      denoise_coef=U.AUX_COEF if opts.aux else 0.0)))
    alg = U._alg(monkeypatch, precision, N, T, symmetry)
    net = alg.net
    assert (net.shadow_ld(0) > 0) == (precision == "bf16") and (net.obs_norm is not None) == opts.norm
    assert alg._ppo_cfg.value_loss_unclipped == int(opts.unclipped) and (alg._ppo_cfg.aux_coef > 0) == opts.aux
    g = torch.Generator().manual_seed(5)
    sigma = torch.where(torch.arange(12) % 2 == 0, 0.5 + 0.3 * torch.rand(12, generator=g), 1.3 + 0.3 * torch.rand(12, generator=g))
    net.views[list(net.views)[0]].copy_((torch.log(sigma) if opts.std == "log" else sigma).cuda())
    net.sync_shadow()
    stats = None
    if opts.norm:
        stats = U.unit_row_stats((705, 219), g)
        net.load_norm_state(U.norm_state_of(stats))
        net.sync_shadow()
    torch.cuda.synchronize()
    return alg, stats


MARGIN = 0.03


def _defuse(alg, opts, params, stats, spec):
    """A drawn rollout puts the MIRRORED copy of a row anywhere: its ratio and its |V - V_old| may land on a clip bound, where the loss's
    gradient jumps and a kernel and a reference that agree to 1e-3 may take different branches -- a whole row's gradient among 256.
    (make_case keeps its rows away from the bounds by construction; the original copies here sit at ratio 1, V = V_old.)  Rows either of
    whose copies comes within MARGIN of a ratio bound get advantage 0 (no surrogate term on either side of the bound); rows whose
    |V - V_old| comes within MARGIN of clip get their returns placed 1 beyond V_old on the side where the unclipped branch wins on both
    sides of the bound (V above V_old: returns below both).  The inputs change, the update under test does not.  -> rows changed."""
    st = alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    fl = lambda t: t.flatten(0, 1).clone().cpu()
    cols = U.mirror_columns([fl(st.observations), fl(st.privileged_observations), fl(st.actions), st.values.flatten().clone().cpu(),
                             st.advantages.flatten().clone().cpu(), st.returns.flatten().clone().cpu(), st.actions_log_prob.flatten().clone().cpu(),
                             fl(st.mu), fl(st.sigma)], spec)
    mu, v, _ = U.forward(opts, params, stats, cols[0], cols[1])
    log_ratio = P.gaussian_log_prob(cols[2].double(), mu, mu * 0 + U.sigma_of(opts, params)) - cols[6].double()
    clip = float(np.float32(alg.clip_param))
    near_r = ((log_ratio - math.log1p(clip)).abs() < MARGIN) | ((log_ratio - math.log1p(-clip)).abs() < MARGIN)
    d = v - cols[3].double()
    near_v = ((d.abs() - clip).abs() < MARGIN)
    M = T * N
    rows_r = torch.nonzero(near_r[:M] | near_r[M:]).flatten()
    rows_v = torch.nonzero(near_v[:M] | near_v[M:]).flatten()
    assert not bool((near_v[:M] & near_v[M:]).any())
    with torch.inference_mode():
        st.advantages.view(-1)[rows_r.cuda()] = 0.0
        dv = torch.where(near_v[:M], d[:M], d[M:])[rows_v]
        st.returns.view(-1)[rows_v.cuda()] = (cols[3][:M][rows_v].double() - torch.sign(dv)).float().cuda()
    torch.cuda.synchronize()
    return int(rows_r.numel()), int(rows_v.numel())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("other", OTHERS)
def test_update_with_symmetry_and_each_other_option(monkeypatch, other, precision):
    """PPO.update() with symmetry on and one other option (or all of them): the first minibatch's gradient, recorded behind
    hgym_ppo_grad + the unfold, against the reference on update_options_common.mirror_columns(rollout) at the recorded indices.  The
    mirrored half comes from hgym_mirror_rows on the device side and from torch indexing on the reference's."""
    opts = _sym_opts(other, precision)
    spec = _spec()
    alg, stats = _alg_with(monkeypatch, opts, precision, spec)
    st, net, T, N = alg.storage, alg.net, T_SYM, N_SYM
    assert st.mirrored
    U._fill_rollout(alg, 31)
    assert (st.shadows() is not None) == (precision == "bf16")
    params = {k: v.cpu() for k, v in net.state_dict().items()}
    changed = _defuse(alg, opts, params, stats, spec)
    assert changed[0] + changed[1] < T * N // 4, changed
    fl = lambda t: t.flatten(0, 1).clone().cpu()
    cols0 = [fl(st.observations), fl(st.privileged_observations), fl(st.actions), st.values.flatten().clone().cpu(), st.advantages.flatten().clone().cpu(),
             st.returns.flatten().clone().cpu(), st.actions_log_prob.flatten().clone().cpu(), fl(st.mu), fl(st.sigma)]
    idx_log, grad_log = U._record_batches(monkeypatch, alg)
    unfold_log, unfold = [], net.norm_unfold_grad

    def uf():
        unfold()
        unfold_log.append(net.grads.clone())
    monkeypatch.setattr(net, "norm_unfold_grad", uf)
    alg.update()
    torch.cuda.synchronize()
    assert len(idx_log) == 2 and idx_log[0].numel() == T * N and len(unfold_log) == (2 if opts.norm else 0)
    idx = idx_log[0]
    rows = torch.where(idx >= (T + 1) * N, idx - N, idx).contiguous().cpu()      # plain row numbers of [0, 2 T N)
    assert int((rows >= T * N).sum()) > 0 and int((rows < T * N).sum()) > 0
    flat = (unfold_log if opts.norm else grad_log)[0].cpu()
    base = net.params.data_ptr()
    got = {k: flat[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v) for k, v in net.views.items()}
    ppo = dict(clip=float(np.float32(alg.clip_param)), value_coef=float(np.float32(alg.value_loss_coef)),
               entropy_coef=float(np.float32(alg.entropy_coef)), aux_coef=float(np.float32(U.AUX_COEF)) if opts.aux else 0.0)
    ref = U.reference(opts, params, stats, U.mirror_columns(cols0, spec), rows, ppo)
    _hold("symmetry x %s, %s: first minibatch's gradient vs float64 reference on torch-mirrored columns" % (other, precision), opts,
          U.errors(opts, got, ref), U.bar_of(opts))
    # the mirrored half matters: the reference on the original rows alone (each taken where the minibatch took either copy) is far away
    alone = U.reference(opts, params, stats, cols0 + [], torch.where(rows >= T * N, rows - T * N, rows), ppo)
    moved = U.errors(opts, {k: g for k, g in alone["grads"].items()}, ref)
    assert max(moved.values()) > U.SENSITIVITY * U.bar_of(opts), moved


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_normaliser_merges_the_original_rows_only(monkeypatch, precision):
    """Symmetry + normalisation: after update() the statistics are obs_norm_common.merge(planted, the T N ORIGINAL rows) within
    tests/test_obs_norm_gpu.py::test_accumulate_and_merge_against_float64's bounds, the count grew by T N (not 2 T N), and a twin
    without symmetry on the same rollout ends with the same bits."""
    opts = _sym_opts("norm", precision)
    T, N = T_SYM, N_SYM
    states = {}
    for name, symmetry in (("on", _spec()), ("off", None)):
        alg, stats = _alg_with(monkeypatch, opts, precision, symmetry)
        assert alg.storage.mirrored == (symmetry is not None)
        U._fill_rollout(alg, 33)
        rows = [alg.storage._obs_all[:T].flatten(0, 1).clone().cpu().numpy(), alg.storage._priv_all[:T].flatten(0, 1).clone().cpu().numpy()]
        alg.update()
        torch.cuda.synchronize()
        states[name] = alg.net.norm_state()
        monkeypatch.undo()
        if symmetry is None:
            continue
        for k, key in enumerate(("obs", "critic_obs")):
            got = states[name][key]
            ref = ON.merge(dict(mean=stats["mean"][k], var=stats["var"][k], count=U.PLANTED_COUNT), rows[k])
            dm, dv = ON.bounds(rows[k])
            assert float(got["count"]) == U.PLANTED_COUNT + T * N == ref["count"]
            em = np.abs(got["mean"].cpu().numpy() - ref["mean"]).max()
            ev = np.abs(got["var"].cpu().numpy() - ref["var"]).max()
            print("%s %s: |d mean| %.3e (bound %.3e)  |d var| %.3e (bound %.3e)" % (precision, key, em, dm, ev, dv))
            assert em <= dm and ev <= dv
            # ... and not the merge of the doubled rows (the mirrored copies negate columns: their mean would be pulled towards 0)
            doubled = ON.merge(dict(mean=stats["mean"][k], var=stats["var"][k], count=U.PLANTED_COUNT), np.concatenate((rows[k], -rows[k])))
            assert np.abs(doubled["mean"] - ref["mean"]).max() > 1e3 * dm
    for key in ("obs", "critic_obs"):
        a, b = states["on"][key], states["off"][key]
        assert float(a["count"]) == float(b["count"])
        for part in ("mean", "var"):
            assert torch.equal(a[part].view(torch.int64), b[part].view(torch.int64)), (key, part)


# ---------------------------------------------------------------------------------------------- e. the runner
TASK, N_RUN, T_RUN = "humanoid_dwl_ppo", 64, 8


def _runner(monkeypatch, log_root, seed=57):
    import sys
    from humanoid.algo import OnPolicyRunner, PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    monkeypatch.setattr(PPO, "precision", "bf16")
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(N_RUN), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    train_cfg.runner.num_steps_per_env = T_RUN
    train_cfg.runner.save_interval = 1
    train_cfg.runner.exact_resume = True
    train_cfg.algorithm.symmetry = True
    train_cfg.algorithm.use_clipped_value_loss = False
    train_cfg.policy.noise_std_type = "log"
    train_cfg.policy.empirical_normalization = True
    R = sys.modules[OnPolicyRunner.__module__]
    AC = getattr(R, "_uo_AC", None) or R.ActorCritic
    monkeypatch.setattr(R, "_uo_AC", AC, raising=False)
    # (the activation module is handed in at the constructor: tests/test_fused_activations_gpu.py::_runner)
    monkeypatch.setattr(R, "ActorCritic", lambda *a, **k: AC(*a, **dict(k, activation=U.TANH, fused_activation=True)))
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=str(log_root))
    alg = runner.alg
    assert alg.storage.mirrored and alg._symmetry is not None and alg.net.obs_norm is not None and list(alg.net.views)[0] == "log_std"
    assert alg._ppo_cfg.value_loss_unclipped == 1 and alg._ppo_cfg.aux_coef > 0 and alg.net.cfg.fused_activation == 1
    assert alg.net.shadow_ld(0) == 768 and alg.actor_critic.fused_activation is True and alg.net.cfg.aux_layers > 0
    return runner


def _run_state(r):
    torch.cuda.synchronize()
    net = r.alg.net
    opt = net.opt_state.clone()
    if float(opt[L.OPT_GRAD_SQNORM]) >= 128.0:      # fp64 atomics beyond their exact range (tests/test_fused_gpu.py)
        opt[L.OPT_GRAD_SQNORM] = 0.0
    ns = net.norm_state()
    return dict(params=net.params.clone(), obs0=r.alg.storage._obs_all[0].clone(), opt_state=opt, adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), sigma=net.sigma.clone(),
                **{"%s.%s" % (k, p): torch.as_tensor(ns[k][p]).clone() for k in ns for p in ("mean", "var", "count")})


def _same(a, b):
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


def test_runner_with_everything_on_captured_as_eager(monkeypatch, tmp_path):
    """humanoid_dwl_ppo (the auxiliary head), 64 envs, 8 steps, 3 iterations with symmetry, log std, normalisation, the unclipped value
    loss and tanh on the fused kernels: the captured update (HGYM_GRAPH_UPDATE=1) against the eager one bit for bit; then an exact resume
    from the checkpoint behind iteration 2 continues into the uninterrupted run's third iteration, bit for bit."""
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", mode)
        torch.manual_seed(4321)
        np.random.seed(4321)
        r = _runner(monkeypatch, tmp_path / ("u" + mode))
        r.learn(num_learning_iterations=3, init_at_random_ep_len=True)
        r.wait_for_saves()
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (mode == "1")
        alg = r.alg
        assert int(alg.net.opt_state[L.OPT_STEP]) == 3 * alg.num_learning_epochs * alg.num_mini_batches
        runs[mode] = _run_state(r)
        for k, t in runs[mode].items():
            assert torch.isfinite(t).all(), (mode, k)
        assert float(runs[mode]["obs.count"]) == 3 * T_RUN * N_RUN and bool((runs[mode]["sigma"] > 0).all())
        if mode == "1":
            path = os.path.join(r.log_dir, "model_1.pt")
            assert os.path.exists(path)
        del r
    assert _same(runs["1"], runs["0"]) == []
    monkeypatch.setenv("HGYM_GRAPH_UPDATE", "1")
    torch.manual_seed(4321)
    np.random.seed(4321)
    r = _runner(monkeypatch, tmp_path / "r")
    r.load(path)
    assert r.current_learning_iteration == 2 and float(r.alg.net.norm_view("header")[2]) == 2 * T_RUN * N_RUN
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(runs["1"], _run_state(r)) == []
