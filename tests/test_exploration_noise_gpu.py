"""-m gpu: PPO.exploration_noise on the device.

hgym_policy_noise_table:
  * identity filter: row t of the table fed to hgym_policy_act gives the actions and log-probabilities of the call with z = NULL at step
    s0 + t, on the smallest fused bf16 net and on the fp32 layer path, with the step's high word changing inside the table
  * filtered tables (colored beta = 1, ar1 rho = 0.9 from a random state) have the bits of the fp32 twin and lie within (t + 2) 2^-24
    sum |coef * w| of float64; the state written is x_{T-1}; two calls continue one process; guard bands stay clean
through the drop-in stack (64 / 128 envs, rollouts of 4 steps, 3 iterations):
  * rho = 0 against the option off: the same parameters and storage under every loop plan
  * rho = 0.9 and beta = 0.5: every loop plan the same bits, actions = mu + sigma * table, exact resume, the refusal of 129 steps
  * the sample lag-1 correlation of one rollout against the configured one
  * a Distillation run: the identity filter against the option off, AR(1) actions = mu + sigma * table"""
import copy
import ctypes as C
import os

import pytest
import torch

from hgym import _lib as L
from humanoid.algo.ppo import exploration_noise as EN
import guard_common as GC

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SEED = 0x1234ABCD5678EF01
S0 = 2 ** 32 - 1
KNOBS = ("HGYM_GRAPH_UPDATE", "HGYM_FUSE_ROLLOUT", "HGYM_GRAPH", "HGYM_ASYNC", "HGYM_ROLLOUT_CRITIC", "HGYM_LOG_SINK", "HGYM_ASYNC_SAVE")


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield
    from humanoid.algo import PPO
    PPO.precision = "bf16"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(T, n, A, filt, carry, state, step, z=None, seed=SEED):
    """One hgym_policy_noise_table call; filt (T, T) / carry (T,) / state (n, A) fp32 device tensors (or None), step a device int64."""
    z = torch.full((T, n, A), float("nan"), device="cuda") if z is None else z
    L.check(L.lib.hgym_policy_noise_table(T, n, A, L.fptr(filt), filt.shape[1], L.fptr(carry), L.fptr(state), seed, L.i64ptr(step), L.fptr(z),
                                          _stream()), "hgym_policy_noise_table")
    return z


def _step(s):
    return torch.tensor([s], dtype=torch.int64, device="cuda")


def _eye(T):
    return torch.eye(T, device="cuda")


def _filters(kind, value, T):
    filt, carry = EN.build_filter(EN.parse_config({"kind": kind, EN.KINDS[kind][0]: value}), T)
    return filt.float().cuda().contiguous(), None if carry is None else carry.float().cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. identity filter
def _net(precision):
    from hgym import NetBuffers, make_net_config
    net = NetBuffers(make_net_config(705, 219, 12, [256, 128, 128], [256, 128, 128], precision, 128), "cuda")
    g = torch.Generator().manual_seed(3)
    with torch.inference_mode():
        net.params.copy_((torch.randn(net.P, generator=g) * 0.05).cuda())
        net.params[:12] = torch.linspace(0.3, 1.4, 12).cuda()      # std
    net.sync_shadow()
    return net


@pytest.mark.parametrize("M", [1, 33, 65])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_identity_table_rows_are_the_policy_launch_own_draws(precision, M):
    T = 3
    net = _net(precision)
    assert (net.shadow_ld(0) > 0) == (precision == "bf16")      # the fused bf16 kernels / the layer-by-layer path
    g = torch.Generator().manual_seed(M)
    obs, priv = torch.randn(M, 705, generator=g).cuda(), torch.randn(M, 219, generator=g).cuda()
    table = _table(T, M, 12, _eye(T), None, None, _step(S0))
    assert torch.isfinite(table).all()
    for t in range(T):
        own = net.act(obs, priv, seed=SEED, step_counter=_step(S0 + t))
        fed = net.act(obs, priv, z=table[t].contiguous(), seed=SEED ^ 0xFFFF, step_counter=_step(12345))      # (neither is read with z)
        torch.cuda.synchronize()
        assert torch.equal(own["actions"], fed["actions"]) and torch.equal(own["logp"], fed["logp"]), (precision, M, t)
        # and the table row IS (a - mu) / sigma up to the epilogue's two roundings
        zz = (own["actions"] - own["mu"]) / own["sigma"]
        assert float((zz - table[t]).abs().max()) <= 1e-4 * (1.0 + float(table[t].abs().max()))
    assert not torch.equal(table[0], table[1]) and not torch.equal(table[1], table[2])


# ------------------------------------------------------------------------------------------------ 2. filtered tables
SHAPES = [(1, 1, 12), (2, 33, 12), (3, 31, 1), (5, 64, 3), (60, 65, 12), (128, 32, 4), (128, 65, 12)]


def _check_against_twins(z, filt, carry, state0, w):
    x32, _ = EN.table_reference(filt.cpu(), None if carry is None else carry.cpu(), None if state0 is None else state0.cpu(), w.cpu(), torch.float32)
    x64, b64 = EN.table_reference(filt.cpu(), None if carry is None else carry.cpu(), None if state0 is None else state0.cpu(), w.cpu(), torch.float64)
    zc = z.cpu()
    assert torch.equal(zc, x32), "max |kernel - fp32 twin| = %g" % float((zc - x32).abs().max())
    steps = (torch.arange(z.shape[0], dtype=torch.float64) + 2.0).view(-1, 1, 1)
    assert bool(((zc.double() - x64).abs() <= steps * U * b64).all())


@pytest.mark.parametrize("T,n,A", SHAPES)
def test_filtered_tables_have_the_twin_bits(T, n, A):
    step = _step(S0 - 1)
    w = _table(T, n, A, _eye(T), None, None, step)      # the raw draws
    torch.cuda.synchronize()
    assert torch.isfinite(w).all()
    if T * n * A >= 1000:      # they are standard normals
        assert abs(float(w.mean())) < 5.0 / (T * n * A) ** 0.5 and abs(float(w.std()) - 1.0) < 0.1
    filt, carry = _filters("colored", 1.0, T)
    assert carry is None
    _check_against_twins(_table(T, n, A, filt, None, None, step), filt, None, None, w)
    filt, carry = _filters("ar1", 0.9, T)
    state0 = torch.randn(n, A, generator=torch.Generator().manual_seed(T * n + A)).cuda()
    state = state0.clone()
    z = _table(T, n, A, filt, carry, state, step)
    torch.cuda.synchronize()
    _check_against_twins(z, filt, carry, state0, w)
    assert torch.equal(state, z[T - 1]) and not torch.equal(state, state0)
    # without a carry the state is not read (NaN would poison the table), and still receives x_{T-1}
    state.fill_(float("nan"))
    z = _table(T, n, A, filt, None, state, step)
    torch.cuda.synchronize()
    _check_against_twins(z, filt, None, None, w)
    assert torch.equal(state, z[T - 1])


# ------------------------------------------------------------------------------------------------ 3. AR(1) continuity
def test_two_calls_continue_one_process():
    """Two tables of 4 steps, the step advanced by 4 and the state handed on, against one table of 8 steps from the same state: every
    entry, and the state left behind (row 7), within (t + 2) 2^-24 B[t], B[t] = sum |coef * term| of row t of the 8-step process in float64."""
    n, A, rho = 33, 12, 0.9
    f8, c8 = _filters("ar1", rho, 8)
    state0 = torch.randn(n, A, generator=torch.Generator().manual_seed(5)).cuda()
    w = _table(8, n, A, _eye(8), None, None, _step(S0 - 5))
    one_state = state0.clone()
    one = _table(8, n, A, f8, c8, one_state, _step(S0 - 5))
    two_state = state0.clone()
    a = _table(4, n, A, f8, c8, two_state, _step(S0 - 5))       # (the leading block of the 8-step filter)
    b = _table(4, n, A, f8, c8, two_state, _step(S0 - 1))
    torch.cuda.synchronize()
    two = torch.cat([a, b])
    assert torch.equal(two[:4], one[:4]) and torch.equal(two_state, b[3]) and torch.equal(one_state, one[7])
    _, b64 = EN.table_reference(f8.cpu(), c8.cpu(), state0.cpu(), w.cpu(), torch.float64)
    bound = (torch.arange(8, dtype=torch.float64) + 2.0).view(-1, 1, 1) * U * b64
    diff = (two.cpu().double() - one.cpu().double()).abs()
    print("max |two calls - one call| / bound = %.3f (largest difference %.3g)" % (float((diff / bound).max()), float(diff.max())))
    assert bool((diff <= bound).all())
    assert bool(((two_state.cpu().double() - one_state.cpu().double()).abs() <= bound[7]).all())


# ------------------------------------------------------------------------------------------------ 4. guard bands
@pytest.mark.parametrize("T,n,A", [(3, 33, 12), (128, 65, 12)])
def test_guard_bands_stay_clean(T, n, A):
    filt, carry = _filters("ar1", 0.9, T)
    sizes = [4 * T * n * A, 4 * n * A, 4 * T * T, 4 * T, 8]
    arena = GC.Arena("cuda", GC.arena_bytes(*sizes))
    z = arena.carve((T, n, A), torch.float32, name="z")
    state = arena.place(torch.randn(n, A, generator=torch.Generator().manual_seed(9)).cuda(), name="state")
    gf, gc_, step = arena.place(filt, name="filt"), arena.place(carry, name="carry"), arena.place(_step(S0 - 2), name="step")
    state0 = state.clone()
    w = _table(T, n, A, _eye(T), None, None, step)
    _table(T, n, A, gf, gc_, state, step, z=z)
    torch.cuda.synchronize()
    arena.verify("hgym_policy_noise_table (%d, %d, %d)" % (T, n, A))
    assert torch.isfinite(z).all()
    _check_against_twins(z, filt, carry, state0, w)
    assert torch.equal(state, z[T - 1])


# ------------------------------------------------------------------------------------------------ 5.-7. the drop-in stack
T_RUN, ITS = 4, 3
PLANS = {      # the loop plans of OnPolicyRunner.learn: how the rollout is launched x whether it is captured
    "stepwise": dict(HGYM_FUSE_ROLLOUT="0"), "stepwise-eager": dict(HGYM_FUSE_ROLLOUT="0", HGYM_GRAPH="0"),
    "inline": dict(HGYM_ROLLOUT_CRITIC="inline"), "inline-eager": dict(HGYM_ROLLOUT_CRITIC="inline", HGYM_GRAPH="0"),
    "deferred": dict(HGYM_ROLLOUT_CRITIC="deferred"), "deferred-eager": dict(HGYM_ROLLOUT_CRITIC="deferred", HGYM_GRAPH="0"),
}


def _runner(N, noise=None, tmp=None, steps=T_RUN, seed=31, exact=False, save_interval=50):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", str(N), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="humanoid_ppo"))
    env_cfg.seed = train_cfg.seed = seed
    env_cfg.env.episode_length_s = 4                 # 400-step episodes: resets (and time-outs) inside the rollouts
    train_cfg.runner.num_steps_per_env = steps
    train_cfg.runner.save_interval = save_interval
    train_cfg.algorithm.num_learning_epochs, train_cfg.algorithm.num_mini_batches = 2, 2
    if exact:
        train_cfg.runner.exact_resume = True
    if noise is not None:
        train_cfg.algorithm.exploration_noise_cfg = noise
    env, _ = task_registry.make_env(name="humanoid_ppo", args=args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, name="humanoid_ppo", args=args, train_cfg=train_cfg, log_root=None if tmp is None else str(tmp))
    assert PPO.exploration_noise is None
    return runner


def _state(runner):
    torch.cuda.synchronize()
    net, st = runner.alg.net, runner.alg.storage
    cols = [getattr(st, k).clone() for k in ("actions", "mu", "sigma", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages")]
    return [net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.opt_state[L.OPT_LR:L.OPT_STEP + 1].clone(), st._obs_all.clone(),
            st._priv_all.clone()] + cols


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _same(a, b):
    return len(a) == len(b) and all(_bits(x, y) for x, y in zip(a, b))


def _run(monkeypatch, plan, N, noise, its=ITS):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    r = _runner(N, noise)
    r.learn(num_learning_iterations=its, init_at_random_ep_len=True)
    fused = plan.split("-")[0]
    if fused != "stepwise":      # the plan that was asked for is the plan that ran
        assert r.env.rollout_fused_mode(r.alg.net) == fused
    assert (r._graph is not None) == (not plan.endswith("eager"))
    return r


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("plan", list(PLANS))
def test_identity_filter_is_the_option_off(monkeypatch, plan, N):
    """rho = 0 builds the exact identity: the table launch runs, every policy launch reads its row, and the parameters and the storage are
    those of a run without the option, bit for bit (at 128 envs the inline plan reaches the 64-row critic layout)."""
    on = _run(monkeypatch, plan, N, {"kind": "ar1", "rho": 0.0})
    assert on.alg._noise is not None and on.alg._noise.state is None and on.alg._noise.table.shape == (T_RUN, N, 12)
    assert on.alg.rollout_graph_key()[-1][0] == "exploration_noise" and dict(on.alg.log_scalars()) == {"Policy/noise_lag1": 0.0}
    assert on.alg.log_scalars() == []      # (logged once)
    s_on = _state(on)
    table = on.alg._noise.table.clone()
    off = _run(monkeypatch, plan, N, None)
    assert off.alg._noise is None and off.alg._scalar_order == () and len(off.alg.rollout_graph_key()) == 3
    assert _same(s_on, _state(off)), "plan %s, %d envs: the identity filter left the run without the option" % (plan, N)
    assert torch.isfinite(table).all() and float(table.abs().max()) > 1.0


_REFERENCE = {}


def _reference(monkeypatch, key, N, noise):
    """The stepwise eager run of a filter: computed once, shared by the plans compared with it, never changed."""
    if key not in _REFERENCE:
        r = _run(monkeypatch, "stepwise-eager", N, noise)
        _REFERENCE[key] = (_state(r), r.alg._noise.table.clone(), None if r.alg._noise.state is None else r.alg._noise.state.clone())
    return _REFERENCE[key]


FILTERS = {"ar1-0.9": {"kind": "ar1", "rho": 0.9}, "colored-0.5": {"kind": "colored", "beta": 0.5}}


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("plan", [p for p in PLANS if p != "stepwise-eager"] + ["stepwise-eager"])
def test_real_filters_agree_across_loop_plans(monkeypatch, plan, name):
    N, noise = 64, FILTERS[name]
    ref_state, ref_table, ref_noise_state = _reference(monkeypatch, name, N, noise)
    r = _run(monkeypatch, plan, N, noise)
    alg, st = r.alg, r.alg.storage
    assert _same(ref_state, _state(r)), "%s: plan %s left the stepwise eager run" % (name, plan)
    assert _bits(ref_table, alg._noise.table) and (ref_noise_state is None or _bits(ref_noise_state, alg._noise.state))
    # the stored actions are mu + sigma * x in plain fp32 (two roundings), x the table of the last rollout
    assert torch.equal(st.actions, st.mu + st.sigma * alg._noise.table)
    assert (alg._noise.state is None) == (noise["kind"] == "colored")
    if alg._noise.state is not None:
        assert torch.equal(alg._noise.state, alg._noise.table[T_RUN - 1])
    # and the noise is not white: consecutive rows correlate
    x = alg._noise.table
    corr = float((x[:-1] * x[1:]).mean())
    assert corr > 0.15, corr


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("async_save", ["1", "0"], ids=["background-save", "blocking-save"])
def test_exact_resume_continues_the_sequence(tmp_path, monkeypatch, name, async_save):
    """2 + 2 iterations through a checkpoint with its sidecar equal 4 iterations; the AR(1) state rides in the sidecar on both save paths;
    model_<it>.pt has the reference's keys and loads under any noise setting."""
    noise = FILTERS[name]
    monkeypatch.setenv("HGYM_ASYNC_SAVE", async_save)
    u = _runner(64, noise, tmp_path / "u", exact=True, save_interval=1)
    u.learn(num_learning_iterations=4, init_at_random_ep_len=True)
    u.wait_for_saves()
    final = _state(u)
    model, side_path = os.path.join(u.log_dir, "model_1.pt"), os.path.join(u.log_dir, "envstate_1.pt")
    assert list(torch.load(model, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict", "iter", "infos"]
    side = torch.load(side_path, map_location="cpu")
    if noise["kind"] == "ar1":
        sd = side[EN.SIDECAR_KEY]
        assert sd["kind"] == "ar1" and sd["value"] == 0.9 and sd["state"].shape == (64, 12) and torch.isfinite(sd["state"]).all()
    else:
        assert EN.SIDECAR_KEY not in side
    r = _runner(64, noise, tmp_path / "r", exact=True)
    before = None if r.alg._noise.state is None else r.alg._noise.state.clone()
    r.load(model)
    assert r.current_learning_iteration == 2
    if before is not None:
        assert not torch.equal(before, r.alg._noise.state) and torch.equal(r.alg._noise.state.cpu(), side[EN.SIDECAR_KEY]["state"])
    r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    r.wait_for_saves()
    assert _same(final, _state(r)), "%s: the resumed run left the uninterrupted one" % name
    # the model file knows nothing of the option: it loads into a run without it, and one of a run without it loads here
    plain = _runner(64, None, tmp_path / "p")
    plain.load(model, env_state=False)
    plain.save(str(tmp_path / "plain.pt"))
    r.load(str(tmp_path / "plain.pt"))
    if noise["kind"] == "ar1":      # a sidecar whose state does not fit is refused before anything is changed
        side[EN.SIDECAR_KEY]["state"] = side[EN.SIDECAR_KEY]["state"][:32]
        torch.save(side, tmp_path / "short.pt")
        with pytest.raises(ValueError, match="exploration noise state: shape"):
            r.load(model, env_state=str(tmp_path / "short.pt"))


def test_refusals():
    with pytest.raises(ValueError, match="num_steps_per_env=129 exceeds the 128"):
        _runner(32, {"kind": "colored", "beta": 0.5}, steps=129)
    with pytest.raises(ValueError, match="unknown key 'gain'"):
        _runner(32, {"kind": "ar1", "rho": 0.5, "gain": 2.0})
    with pytest.raises(ValueError, match="outside"):
        _runner(32, {"kind": "ar1", "rho": 1.0})
    _runner(32, None, steps=129)      # without the option the storage may be as long as it likes


# ------------------------------------------------------------------------------------------------ 7. lag-1 statistic
@pytest.mark.parametrize("name", list(FILTERS))
def test_sample_lag1_correlation_is_the_configured_one(name):
    """(a - mu) / sigma over one rollout of 128 envs x 24 steps: the sample lag-1 correlation within 6 standard errors of r(1), the standard
    error that of a product of two unit normals with correlation r, sqrt((1 + r^2) / samples).  The seed is fixed, so the outcome is too."""
    N, T = 128, 24
    r = _runner(N, FILTERS[name], steps=T)
    r.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    st, noise = r.alg.storage, r.alg._noise
    x = ((st.actions - st.mu) / st.sigma).double()
    assert float((x - noise.table.double()).abs().max()) <= 1e-4 * (1.0 + float(noise.table.abs().max()))
    a, b = x[:-1].flatten(), x[1:].flatten()
    corr = float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))
    r1 = noise.lag1
    assert r1 == EN.lag1(EN.parse_config(FILTERS[name]), T) and 0.2 < r1 <= 0.9
    se = ((1.0 + r1 * r1) / a.numel()) ** 0.5
    print("%s: sample lag-1 correlation %.4f, configured %.4f, standard error %.4f (%d pairs)" % (name, corr, r1, se, a.numel()))
    assert abs(corr - r1) <= 6.0 * se
    assert abs(float(x.mean())) <= 6.0 / x.numel() ** 0.5 * 3 and abs(float(x.var()) - 1.0) <= 0.1      # the marginal stays N(0, 1)


# ------------------------------------------------------------------------------------------------ with Distillation
def test_distillation_samples_from_the_table(tmp_path):
    """A cloning run collects with the student's sampled actions through the same PPO.act / one-launch rollout: with rho = 0 the student's
    parameters and the stored actions are those of a run without the option; with rho = 0.9 the stored actions are mu + sigma * table."""
    import test_distillation_gpu as TD
    from humanoid.algo import Distillation
    path = str(tmp_path / "teacher.pt")
    TD._runner("humanoid_ppo", None, seed=3).save(path)
    runs = {}
    for name, noise in (("identity", {"kind": "ar1", "rho": 0.0}), ("off", None), ("ar1", {"kind": "ar1", "rho": 0.9})):
        r = TD._runner("humanoid_distill", None, **({} if noise is None else {"exploration_noise_cfg": noise}))
        r.load(path)
        r.learn(num_learning_iterations=2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert isinstance(r.alg, Distillation) and (r.alg._noise is None) == (noise is None)
        runs[name] = r
    a, b, c = runs["identity"].alg, runs["off"].alg, runs["ar1"].alg
    assert _bits(a.net.params, b.net.params) and _bits(a.storage.actions, b.storage.actions) and _bits(a.storage._obs_all, b.storage._obs_all)
    assert torch.equal(c.storage.actions, c.storage.mu + c.storage.sigma * c._noise.table) and not _bits(c.storage.actions, b.storage.actions)
