"""-m gpu: the measurement hooks of include/hgym.h (hgym_prof_phase_buffer, hgym_prof_enable / hgym_prof_summary) do not write out of bounds,
do not change what they observe, and report the work the documentation says they report.

The phase buffer.  Every fused kernel stores into the caller's buffer at (blockIdx.y * gridDim.x + blockIdx.x) * 8 + slot, behind pointer
offsets the host adds per launch.  The buffer here is carved from a tests/guard_common.py Arena (int64, contents 0xFF... = -1) with
EXACTLY the number of slots the launch asks for; every other pointer of the call is an ordinary tensor (tests/test_guard_bands_gpu.py guards
those).  The expected grids come from guard_common.phase_groups, which tests/test_guard_bands.py holds to hand-computed values.  Per launch
of G groups:
  1  exact size     8 G slots: the bands stay clean, at least one slot changed
  2  one slot short 8 G - 1 slots declared (same carve): no slot changes -- the library declines, the kernel never sees a smaller buffer
  3  off            after hgym_prof_phase_buffer(NULL, 0) no slot changes
  4  no observer effect: every output of 1 and 2 has the bits of the uninstrumented call
  5  the stamps: positive; exactly the slots of the workgroups that stamp have changed; non-decreasing in slot order within one writer;
     no writer's span, and not the whole launch's, is longer than the host's perf_counter interval around launch + synchronise in 100 MHz
     ticks (no margin: the host interval contains the launch)
  6  the 64-row rollout launch at N = 320: exactly N / 64 non-actor groups carry the side-job pattern, at the swapped columns

Not tested: a HIP graph capture with the hooks on (the header says they are not capturable)."""
import ctypes as C
import time

import pytest
import torch

import guard_common as G
import test_guard_bands_gpu as GB
import update_options_common as U
from hgym import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F64, I64 = torch.bfloat16, torch.float64, torch.int64
TICKS_PER_SECOND = 1e8          # s_memrealtime: the 100 MHz wall clock


@pytest.fixture
def hooks():
    """The hook state is process-global: whatever the test does, it ends with the phase buffer unset and profiling off."""
    L.lib.hgym_prof_phase_buffer(None, 0)
    L.lib.hgym_prof_enable(0)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.lib.hgym_prof_phase_buffer(None, 0)
        L.lib.hgym_prof_enable(0)


class PhaseBuffer:
    """8 * groups int64 slots between bands, all -1."""

    def __init__(self, groups):
        self.slots = 8 * int(groups)
        self.arena = G.Arena(DEV, G.arena_bytes(8 * self.slots))
        self.buf = self.arena.carve(self.slots, I64, name="phase buffer of %d slots" % self.slots)
        assert bool((self.buf == -1).all())

    def set(self, slots=None):
        L.check(L.lib.hgym_prof_phase_buffer(C.c_void_p(self.buf.data_ptr()), self.slots if slots is None else int(slots)), "hgym_prof_phase_buffer")

    def off(self):
        L.check(L.lib.hgym_prof_phase_buffer(None, 0), "hgym_prof_phase_buffer")

    def take(self, what):
        """The slots after the call (host copy), the bands verified; the buffer is -1 again."""
        torch.cuda.synchronize()
        self.arena.verify(what)
        v = self.buf.cpu().clone()
        self.buf.fill_(-1)
        return v


def _check_stamps(v, launch, wall_s, what):
    """5 of the module docstring."""
    changed = (v != -1).nonzero().flatten().tolist()
    want = launch.slots()
    assert changed == want, "%s: slots that changed %s, slots the launch's workgroups stamp %s" % (
        what, sorted(set(changed) - set(want)), sorted(set(want) - set(changed)))
    assert changed, what
    vals = v[changed]
    assert bool((vals > 0).all()), "%s: a stamp is not positive" % what
    ticks = wall_s * TICKS_PER_SECOND
    spans = []
    for g, writers in sorted(launch.stamps.items()):
        for w in writers:
            t = [int(v[g * 8 + s]) for s in w]
            assert t == sorted(t), "%s: group %d slots %s are not in program order: %s" % (what, g, w, t)
            spans.append(t[-1] - t[0])
    whole = int(vals.max() - vals.min())
    print("%s: %d groups, longest writer %d ticks, launch %d ticks, host %.0f ticks" % (what, len(launch.stamps), max(spans), whole, ticks))
    assert max(spans) <= ticks and whole <= ticks, "%s: %d / %d ticks inside a host interval of %.0f" % (what, max(spans), whole, ticks)


def _phase_entry(what, launch, prepare, call, outputs):
    """1-5 for an entry point that makes ONE phase_buffer request.  prepare(): puts the inputs' state back; call(): enqueues the entry point;
    outputs(): {name: clone of an output}."""
    pb = PhaseBuffer(launch.groups)

    def run(tag):
        prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return pb.take("%s, %s" % (what, tag)), outputs(), wall
    v, ref, _ = run("no buffer set")
    assert bool((v == -1).all())
    pb.set()
    v, got, wall = run("exact size")
    _check_stamps(v, launch, wall, what)
    GB._compare(ref, got, what + ", buffer of the exact size")
    pb.set(pb.slots - 1)
    v, got, _ = run("one slot short")
    assert bool((v == -1).all()), "%s: %d slots changed in a buffer declared one slot short" % (what, int((v != -1).sum()))
    GB._compare(ref, got, what + ", buffer one slot short")
    pb.set()
    pb.off()
    v, got, _ = run("off again")
    assert bool((v == -1).all()), "%s: %d slots changed after hgym_prof_phase_buffer(NULL, 0)" % (what, int((v != -1).sum()))
    GB._compare(ref, got, what + ", off again")


def _cus():
    n = int(L.lib.hgym_device_cus())
    assert n > 0
    return n


def _clones(d):
    return {k: v.clone() for k, v in d.items()}


def _act_io(net, M, seed, shadow=True):
    g = GB._gen(seed)
    A = net.cfg.num_actions
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    obs, priv, z = r(M, net.cfg.num_obs), r(M, net.cfg.num_priv), r(M, A)
    e = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(actions=e(M, A), mu=e(M, A), sigma=e(M, A), logp=e(M), values=e(M, 1))
    sh = (torch.zeros(M, net.shadow_ld(0), dtype=BF16, device=DEV), torch.zeros(M, net.shadow_ld(1), dtype=BF16, device=DEV)) if shadow else None
    return obs, priv, z, out, sh


# ------------------------------------------------------------------------------------------------ forward launches
@pytest.mark.parametrize("M", [1, 33, 65])
@pytest.mark.parametrize("tanh", [False, True], ids=["elu", "tanh"])
def test_phase_policy_act(hooks, M, tanh):
    """hgym_policy_act: mlp_fwd_kernel<32,8,4> on a (tiles, 2) grid; on the Tanh net mlp_fwd_act_kernel, one launch per net behind a host-side
    pointer offset."""
    opts = GB._opts("bf16-fused", act=U.TANH if tanh else None)
    case, net = GB._case(opts), GB._nets(opts)[0]
    obs, priv, z, out, sh = _act_io(net, M, M)
    launch, = G.phase_groups("policy_act", dict(M=M, cus=_cus(), generic=tanh))
    assert launch.groups == 2 * ((M + 31) // 32)
    _phase_entry("hgym_policy_act M=%d %s" % (M, "tanh" if tanh else "elu"), launch, lambda: GB._fresh(net, opts, case),
                 lambda: net.act(obs, priv, z=z, out=out, shadow=sh), lambda: _clones(dict(out, obs_bf16=sh[0], priv_bf16=sh[1])))


def test_phase_policy_act_64_row_tiles(hooks):
    """The smallest M that forces mlp_fwd_kernel<64,16,2>: two nets of ceil(M / 32) 32-row tiles no longer fit the chip's CUs in one round."""
    from hgym import NetBuffers, make_net_config
    cus = _cus()
    M = cus * 16 + 1
    opts = GB._opts("bf16-fused")
    case = GB._case(opts)
    no, npv, A, ah, ch = U.SHAPES["bf16-fused"]["net"]
    net = NetBuffers(make_net_config(no, npv, A, ah, ch, "bf16", M, fused_activation=True), DEV, learning_rate=GB.LR)
    obs, priv, z, out, sh = _act_io(net, M, M)
    launch, = G.phase_groups("policy_act", dict(M=M, cus=cus))
    assert launch.groups == 2 * ((M + 63) // 64) and G.phase_groups("policy_act", dict(M=M - 1, cus=cus))[0].groups == 2 * ((M - 1) // 32)
    _phase_entry("hgym_policy_act M=%d (64-row tiles)" % M, launch, lambda: GB._fresh(net, opts, case),
                 lambda: net.act(obs, priv, z=z, out=out, shadow=sh), lambda: _clones(dict(out, obs_bf16=sh[0], priv_bf16=sh[1])))


@pytest.mark.parametrize("M", [1, 33, 65])
def test_phase_policy_act_fin(hooks, M):
    """hgym_policy_act_fin: the same tiles plus the postponed finaliser's grid row, which is counted in the request (3 rows) and stamps nothing.
    The env (37 envs, one deferred step) is put back before every call: the finaliser's effects are outputs too."""
    opts = GB._opts("bf16-fused")
    case, net = GB._case(opts), GB._nets(opts)[0]
    side = GB.Side("hgym_policy_act_fin", G.Plain(DEV), net)
    cfg, buf = GB._make_env(side, 37, "soa")
    sim, st, o = buf.sim_struct(), buf.state_struct(), buf.out_struct()
    nz = buf.noise_struct()
    L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), GB._s()), "hgym_env_prime")
    GB._plant(buf, 37)
    od = buf.out_struct(defer_finalize=True)
    a = torch.randn(37, 12, generator=GB._gen(3)).to(DEV)
    L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(od), L.fptr(a), GB._s()), "hgym_env_step_synth")
    torch.cuda.synchronize()
    own = {k: t for k, t in vars(buf).items() if torch.is_tensor(t) and t._base is None}
    saved = _clones(own)
    obs, priv, z, out, sh = _act_io(net, M, M + 7)

    def prepare():
        GB._fresh(net, opts, case)
        for k, t in own.items():
            t.copy_(saved[k])
    launch, = G.phase_groups("policy_act", dict(M=M, cus=_cus(), fin=True))
    assert launch.groups == 3 * ((M + 31) // 32)
    _phase_entry("hgym_policy_act_fin M=%d" % M, launch, prepare, lambda: net.act(obs, priv, z=z, out=out, env_fin=(cfg, st, od), shadow=sh),
                 lambda: GB._env_state(buf, _clones(dict(out, obs_bf16=sh[0], priv_bf16=sh[1])), "env."))
    assert int(buf.counters[L.CNT_STEP]) == 398, "the finaliser did not run"


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("tanh", [False, True], ids=["elu", "tanh"])
def test_phase_forward_calls(hooks, M, tanh):
    """hgym_mlp_forward(which = 0, 1, 2 -- the fused auxiliary head's wide-head tile) and hgym_critic_values with the shadow: one net per
    launch, ceil(M / 32) groups."""
    opts = GB._opts("bf16-fused", aux=True, act=U.TANH if tanh else None)
    case, net = GB._case(opts), GB._nets(opts)[0]
    no, npv, A = GB._dims(opts)
    g = GB._gen(M + 11)
    launch, = G.phase_groups("mlp_forward", dict(M=M, cus=_cus()))
    assert launch.groups == (M + 31) // 32
    tag = "M=%d %s" % (M, "tanh" if tanh else "elu")
    for which, nin, nout in ((0, no, A), (1, npv, 1), (2, no, U.SHAPES["bf16-fused"]["aux"][1])):
        x = torch.randn(M, nin, generator=g).to(DEV)
        y = torch.full((M, nout), float("nan"), device=DEV)
        _phase_entry("hgym_mlp_forward which=%d %s" % (which, tag), launch, lambda: GB._fresh(net, opts, case),
                     lambda: L.check(L.lib.hgym_mlp_forward(C.byref(net.cfg), C.byref(net.struct), which, M, L.fptr(x), nin, L.fptr(y), GB._s()),
                                     "hgym_mlp_forward"), lambda: dict(y=y.clone()))
    priv = torch.randn(M, npv, generator=g).to(DEV)
    v, sp = torch.full((M,), float("nan"), device=DEV), torch.zeros(M, net.shadow_ld(1), dtype=BF16, device=DEV)
    _phase_entry("hgym_critic_values %s" % tag, launch, lambda: GB._fresh(net, opts, case), lambda: net.critic_values(priv, v, sp),
                 lambda: dict(values=v.clone(), priv_bf16=sp.clone()))


# ------------------------------------------------------------------------------------------------ update launches
S_ROWS = 260
_UPDATE_CASES = {}


def _update_case(opts, B):
    if (opts, B) not in _UPDATE_CASES:
        _UPDATE_CASES[(opts, B)] = U.make_case(opts, S=S_ROWS, B=B, seed=100 + len(_UPDATE_CASES))
    return _UPDATE_CASES[(opts, B)]


def _grad_outputs(net, extra=None):
    out = dict(extra or {})
    out["grads_ext"] = net.grads_ext.clone()
    GB._opt_state(net, out, "opt_state")
    out["raw:workspace"] = net.workspace.clone()      # activations, dZ, slabs, loss partials: everything the launches of the call left
    return out


GRAD_VARIANTS = dict(elu=dict(), aux=dict(aux=True), tanh=dict(act=U.TANH), unclipped=dict(unclipped=True))


@pytest.mark.parametrize("B", [1, 65, 200])
@pytest.mark.parametrize("variant", list(GRAD_VARIANTS))
def test_phase_ppo_grad(hooks, variant, B):
    """hgym_ppo_grad: mlp_fb_kernel on a (tiles, 2) grid, (tiles, 3) with the fused auxiliary head, its unclipped-value-loss code object, and
    mlp_fb_act_kernel's per-net launches on the Tanh net.  Gradient, loss sums and the whole workspace have the uninstrumented call's bits."""
    from hgym import make_batch, make_ppo_config
    opts = GB._opts("bf16-fused", **GRAD_VARIANTS[variant])
    case, net = _update_case(opts, B), GB._nets(opts)[0]
    cols = [t.to(DEV).contiguous() for t in case["cols"]]
    idx = case["idx"].to(DEV)
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"], clipped_value_loss=not opts.unclipped)
    nets = 3 if opts.aux else 2
    launch, = G.phase_groups("ppo_grad", dict(B=B, nets=nets))
    assert launch.groups == nets * ((B + 63) // 64)
    _phase_entry("hgym_ppo_grad %s B=%d" % (variant, B), launch, lambda: GB._fresh(net, opts, case), lambda: net.ppo_grad(ppo, batch),
                 lambda: _grad_outputs(net))


@pytest.mark.parametrize("B", [1, 65, 200])
def test_phase_bc_grad(hooks, B):
    """hgym_bc_grad: mlp_fb_bc_kernel, the actor's tiles alone."""
    from hgym import make_bc_batch, make_bc_config
    opts = GB._opts("bf16-fused")
    case, net = _update_case(opts, B), GB._nets(opts)[0]
    obs, idx = case["cols"][0].to(DEV).contiguous(), case["idx"].to(DEV)
    target = torch.randn(S_ROWS, net.cfg.num_actions, generator=GB._gen(B)).to(DEV)
    sums = torch.zeros(2, dtype=F64, device=DEV)
    batch, bc = make_bc_batch(obs, idx), make_bc_config()

    def prepare():
        GB._fresh(net, opts, case)
        sums.zero_()
    launch, = G.phase_groups("bc_grad", dict(B=B))
    _phase_entry("hgym_bc_grad B=%d" % B, launch, prepare, lambda: net.bc_grad(bc, batch, target, sums), lambda: _grad_outputs(net, dict(sums=sums.clone())))
    assert float(sums[1]) == 1.0


# ------------------------------------------------------------------------------------------------ the rollout step
def _rollout_form(N, deferred, p, critic64):
    if deferred:
        return "deferred_next" if p.prev else "deferred_first"
    if not p.prev:
        return "first"
    return "steady64" if (p.l0_ready is not None and critic64) else "next"


ROLLOUTS = [(64, 3, False), (64, 3, True), (128, 4, False), (320, 4, False)]


@pytest.mark.parametrize("N,T,deferred", ROLLOUTS, ids=["N%d-%s" % (n, "deferred" if d else "inline") for n, _, d in ROLLOUTS])
def test_phase_rollout(hooks, monkeypatch, N, T, deferred):
    """The rollout sequences of tests/test_guard_bands_gpu.py on ordinary tensors, three times: with the buffer of exactly 3 N / 32 groups
    (every hgym_rollout_step launch checked on its own against the form rollout_plan and N imply; the evaluation launch must write nothing),
    with no buffer (the reference bits), and with the buffer declared one slot short.  In grid row 2's groups the env part's slots 0-5 and the
    finaliser row's slots 6 / 7 come from different workgroups and are ordered within each writer only."""
    GB._set_rollout_env(monkeypatch, None)
    opts = GB._opts("bf16-fused")
    case, net = GB._case(opts), GB._nets(opts, max_batch=max(N, GB.MAX_BATCH))[0]
    critic64 = (N // 32) % 2 == 0 and N // 32 >= 4
    X = N // 32
    pb = PhaseBuffer(3 * X)
    what = "fused rollout N=%d %s" % (N, "deferred" if deferred else "inline")
    info, forms = {}, []

    def watch_exact(name, i, call):
        pb.take("%s: the calls in front of %s %d" % (what, name, i))      # (hgym_critic_values stamps too: its bands are checked, its slots dropped)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        v = pb.take("%s: %s %d" % (what, name, i))
        launches = G.phase_groups("rollout_eval_step", dict(N=N)) if name == "hgym_rollout_eval_step" else \
            G.phase_groups("rollout_step", dict(N=N, form=_rollout_form(N, deferred, info["plan"][i], critic64)))
        if not launches:
            assert bool((v == -1).all()), "%s: the evaluation launch wrote %d slots" % (what, int((v != -1).sum()))
            return
        forms.append(_rollout_form(N, deferred, info["plan"][i], critic64))
        assert launches[0].groups == 3 * X
        _check_stamps(v, launches[0], wall, "%s: %s %d (%s)" % (what, name, i, forms[-1]))
        if forms[-1] == "steady64":      # 6: the side-job pattern (slots 0, 1, 2, 7; the fused forward's 3-6 untouched) sits at the swapped columns
            pattern = lambda g: tuple(s for s in range(8) if int(v[g * 8 + s]) != -1)
            side = [x for x in range(X) if pattern((1 - (x & 1)) * X + x) == G.SIDE_SLOTS]
            assert len(side) == N // 64 and side == [x for x in range(X) if ((x ^ (x >> 3)) & 1)], side

    def watch_silent(name, i, call):
        pb.take("%s: the calls in front of %s %d" % (what, name, i))
        call()
        v = pb.take("%s: %s %d" % (what, name, i))
        assert bool((v == -1).all()), "%s: %s %d changed %d slots" % (what, name, i, int((v != -1).sum()))

    run = lambda watch: GB._rollout_sequence(GB.Side(what, G.Plain(DEV), net), N, T, deferred, opts, case, watch=watch, info=info)
    pb.set()
    got = run(watch_exact)
    want_forms = ["deferred_first"] + ["deferred_next"] * (T - 1) if deferred else ["first"] + (["steady64"] if critic64 else ["next"]) * (T - 1)
    assert forms == want_forms, forms
    pb.off()
    ref = run(watch_silent)
    GB._compare(ref, got, what + ", buffer of the exact size")
    pb.set(pb.slots - 1)
    short = run(watch_silent)
    GB._compare(ref, short, what + ", buffer one slot short")


# ------------------------------------------------------------------------------------------------ event profiling
CLASSES = dict(GEMM=L.PROF_GEMM, ENV_STEP=L.PROF_ENV_STEP, GAE=L.PROF_GAE, LOSS=L.PROF_LOSS, MLP_FWD=L.PROF_MLP_FWD, MLP_BWD=L.PROF_MLP_BWD,
               DW=L.PROF_DW, REDUCE=L.PROF_REDUCE, APPLY=L.PROF_APPLY, POLICY=L.PROF_POLICY, ROLLOUT=L.PROF_ROLLOUT, COMM=L.PROF_COMM)


def _profiled(call, want):
    """call() between hgym_prof_enable(1) and the summaries: {class: (launches, work)} must be `want` (every class not named: nothing), each
    class's time positive and no longer than the host interval from enabling to the summary's return.  Then, with profiling off, the same
    call leaves every summary at 0 / 0.0 / 0.0."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    L.check(L.lib.hgym_prof_enable(1), "hgym_prof_enable")
    call()
    got = {k: L.prof_summary(c) for k, c in CLASSES.items()}
    wall_ms = (time.perf_counter() - t0) * 1e3
    L.check(L.lib.hgym_prof_enable(0), "hgym_prof_enable")
    print({k: v for k, v in got.items() if v[0]}, "host %.3f ms" % wall_ms)
    for k, (n, ms, work) in got.items():
        wn, ww = want.get(k, (0, 0.0))
        assert n == wn, "%s: %d launches, expected %d (all: %s)" % (k, n, wn, got)
        if n == 0:
            assert ms == 0.0 and work == 0.0
        else:
            assert 0.0 < ms <= wall_ms, "%s: %.6f ms inside a host interval of %.6f ms" % (k, ms, wall_ms)
            if ww is not None:
                assert work == ww, "%s: work %r, the restated figure %r" % (k, work, ww)
    call()
    torch.cuda.synchronize()
    assert all(L.prof_summary(c) == (0, 0.0, 0.0) for c in CLASSES.values()), "profiling is off, and a summary is not empty"


def _layers(dims):
    return list(zip(dims[:-1], dims[1:]))


def _net_layers(aux=False):
    no, npv, A, ah, ch = U.SHAPES["bf16-fused"]["net"]
    nets = [_layers([no] + ah + [A]), _layers([npv] + ch + [1])]
    if aux:
        xh, xo, _ = U.SHAPES["bf16-fused"]["aux"]
        nets.append(_layers([no] + xh + [xo]))
    return nets


def _fwd_flops(M, nets):
    """Unpadded 2 M K N per layer."""
    return float(sum(2.0 * M * k * n for net in nets for k, n in net))


def _update_flops(B, nets):
    """HGYM_PROF_MLP_FWD of the update tile: the forward's 2 B K N per layer plus the dZ chain's 2 B K N for layers 1, 2, 3 (dX = dZ W)."""
    return _fwd_flops(B, nets) + float(sum(2.0 * B * k * n for net in nets for k, n in net[1:]))


def test_prof_policy_and_update(hooks):
    """hgym_policy_act, hgym_ppo_grad (fused, with the auxiliary head as the third grid row), hgym_ppo_apply and hgym_bc_grad: launches per
    class and `work`.  The optimiser step, counted from adam_body and sqnorm_prologue_kernel: gradient, both moments and the master weight
    read and rewritten (32 B per parameter), two bf16 operand copies stored per WEIGHT (4 B), and -- grad_norm_ready = 0 -- the gradient
    read once more for its norm (4 B per parameter)."""
    from hgym import make_batch, make_bc_batch, make_bc_config, make_ppo_config
    M, B = 65, 200
    opts = GB._opts("bf16-fused", aux=True)
    case, net = _update_case(opts, B), GB._nets(opts)[0]
    GB._fresh(net, opts, case)
    nets = _net_layers(aux=True)
    obs, priv, z, out, _ = _act_io(net, M, 5, shadow=False)
    _profiled(lambda: net.act(obs, priv, z=z, out=out), dict(POLICY=(1, _fwd_flops(M, nets[:2]))))
    cols = [t.to(DEV).contiguous() for t in case["cols"]]
    idx = case["idx"].to(DEV)
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"])
    # REDUCE: one reduce_slabs_kernel launch over every segment (hgym_ppo_grad is part < 0); its work holds the library's split count
    _profiled(lambda: net.ppo_grad(ppo, batch), dict(MLP_FWD=(1, _update_flops(B, nets)), DW=(1, _fwd_flops(B, nets)), REDUCE=(1, None)))
    weights = sum(k * n for layers in nets for k, n in layers)
    assert net.P == weights + sum(n for layers in nets for _, n in layers) + net.cfg.num_actions
    _profiled(lambda: net.ppo_apply(ppo), dict(APPLY=(1, 32.0 * net.P + 4.0 * weights + 4.0 * net.P)))
    ready = make_ppo_config(grad_norm_ready=True, aux_coef=case["ppo"]["aux_coef"])
    _profiled(lambda: net.ppo_apply(ready), dict(APPLY=(1, 32.0 * net.P + 4.0 * weights)))
    target, sums = torch.randn(S_ROWS, 12, generator=GB._gen(1)).to(DEV), torch.zeros(2, dtype=F64, device=DEV)
    bcb, bc = make_bc_batch(cols[0], idx), make_bc_config()
    _profiled(lambda: net.bc_grad(bc, bcb, target, sums), dict(MLP_FWD=(1, _update_flops(B, nets[:1])), DW=(1, _fwd_flops(B, nets[:1])), REDUCE=(1, None)))


@pytest.mark.parametrize("boot", [False, True], ids=["gae", "gae_bootstrap"])
def test_prof_gae(hooks, boot):
    """Bytes per (t, env) from the entry point's argument list: rewards, values (fp32) and dones (u8) read, returns and advantages (fp32)
    written = 17; hgym_gae_bootstrap also reads time_outs (u8) and writes the bootstrapped reward back (fp32) = 22.  (DESIGN.md's 25 B row
    adds adv_normalize_kernel's 8 B, which has no events of its own.)"""
    T, N = 5, 33
    g = GB._gen(9)
    rew, val, last = torch.randn(T, N, generator=g).to(DEV), torch.randn(T, N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    dones, tos = (torch.rand(T, N, generator=g) < 0.2).to(torch.uint8).to(DEV), (torch.rand(T, N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    ret, adv, stats = torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV), L.gae_stats(N, DEV)
    if boot:
        call = lambda: L.check(L.lib.hgym_gae_bootstrap(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dones), L.u8ptr(tos), L.fptr(last), 0.99, 0.95,
                                                        L.fptr(ret), L.fptr(adv), L.f64ptr(stats), GB._s()), "hgym_gae_bootstrap")
    else:
        call = lambda: L.check(L.lib.hgym_gae(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dones), L.fptr(last), 0.99, 0.95, L.fptr(ret), L.fptr(adv),
                                              L.f64ptr(stats), GB._s()), "hgym_gae")
    per = (4 + 4 + 1) + (4 + 4) + ((1 + 4) if boot else 0)
    _profiled(call, dict(GAE=(1, float(T * N * per))))


def _env_step_bytes():
    """SURVEY.md 8d, per env-step: 245 floats of state and sim tensors, the 14 + 2 older frames read, the 15 x 47 / 3 x 73 rows written,
    6 flag bytes."""
    return 4.0 * (245 + 14 * 47 + 2 * 73 + 15 * 47 + 3 * 73) + 6


def test_prof_env_step(hooks):
    N = 37
    side = GB.Side("hgym_env_step_synth", G.Plain(DEV))
    cfg, buf = GB._make_env(side, N, "soa")
    sim, st, o = buf.sim_struct(), buf.state_struct(), buf.out_struct()
    nz = buf.noise_struct()
    L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), GB._s()), "hgym_env_prime")
    a = torch.randn(N, 12, generator=GB._gen(2)).to(DEV)
    assert _env_step_bytes() == 7898.0
    _profiled(lambda: L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), L.fptr(a), GB._s()), "hgym_env_step_synth"),
              dict(ENV_STEP=(1, N * _env_step_bytes())))


def _rollout_step_bytes(N, nets, deferred):
    """The header's HGYM_PROF_ROLLOUT: per env the env step's bytes plus the policy's rows read (obs, priv) and outputs written (actions,
    mu, sigma, logp, value); per launch the bf16 weight fragments the tiles stream, in the padded layout: 16 x 32 blocks of 1 024 B, the
    contraction padded to whole 128-column chunks.  Deferred values: no privileged row, no value, no critic weights."""
    no, npv, A = 705, 219, 12
    per_env = _env_step_bytes() + 4.0 * (no + npv + 3 * A + 2) - (4.0 * (npv + 1) if deferred else 0.0)
    blocks = lambda k, n: -(-n // 16) * 4 * -(-k // 128)
    w = sum(1024.0 * blocks(k, n) for net in (nets[:1] if deferred else nets[:2]) for k, n in net)
    return N * per_env + w


@pytest.mark.parametrize("deferred", [False, True], ids=["inline", "deferred"])
def test_prof_rollout_is_no_observer(hooks, monkeypatch, deferred):
    """A three-step rollout (N = 64) with profiling on: one HGYM_PROF_ROLLOUT interval per hgym_rollout_step and none for the evaluation
    launch, the header's bytes, hgym_critic_values as HGYM_PROF_POLICY launches; and every output has the bits of the run with profiling off."""
    GB._set_rollout_env(monkeypatch, None)
    N, T = 64, 3
    opts = GB._opts("bf16-fused")
    case, net = GB._case(opts), GB._nets(opts)[0]
    what = "fused rollout N=%d, profiling on" % N
    ref = GB._rollout_sequence(GB.Side(what, G.Plain(DEV), net), N, T, deferred, opts, case)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    L.check(L.lib.hgym_prof_enable(1), "hgym_prof_enable")
    got = GB._rollout_sequence(GB.Side(what, G.Plain(DEV), net), N, T, deferred, opts, case)
    n, ms, work = L.prof_summary(L.PROF_ROLLOUT)
    pn, _, pwork = L.prof_summary(L.PROF_POLICY)
    wall_ms = (time.perf_counter() - t0) * 1e3
    L.check(L.lib.hgym_prof_enable(0), "hgym_prof_enable")
    nets = _net_layers()
    assert n == T and work == T * _rollout_step_bytes(N, nets, deferred) and 0.0 < ms <= wall_ms, (n, ms, work, wall_ms)
    assert (pn, pwork) == ((T, T * _fwd_flops(N, nets[1:2])) if deferred else (0, 0.0))
    GB._compare(ref, got, what)


def test_prof_update_is_no_observer(hooks):
    """One hgym_ppo_grad + hgym_ppo_apply with profiling on leaves the bits it leaves with profiling off."""
    from hgym import make_batch, make_ppo_config
    B = 200
    opts = GB._opts("bf16-fused", aux=True)
    case, net = _update_case(opts, B), GB._nets(opts)[0]
    cols = [t.to(DEV).contiguous() for t in case["cols"]]
    idx = case["idx"].to(DEV)
    batch = make_batch(*cols, idx)
    ppo = make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"])

    def run(on):
        GB._fresh(net, opts, case)
        L.check(L.lib.hgym_prof_enable(1 if on else 0), "hgym_prof_enable")
        net.ppo_grad(ppo, batch)
        net.ppo_apply(ppo)
        torch.cuda.synchronize()
        L.check(L.lib.hgym_prof_enable(0), "hgym_prof_enable")
        return _grad_outputs(net, dict(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), sigma=net.sigma.clone()))
    GB._compare(run(False), run(True), "hgym_ppo_grad + hgym_ppo_apply, profiling on")


def test_prof_enable_clears_and_summary_refuses(hooks):
    """hgym_prof_enable(1) clears what an earlier enable collected; hgym_prof_summary refuses a class outside [0, 12) and NULL outputs."""
    opts = GB._opts("bf16-fused")
    case, net = GB._case(opts), GB._nets(opts)[0]
    GB._fresh(net, opts, case)
    obs, priv, z, out, _ = _act_io(net, 33, 1, shadow=False)
    L.check(L.lib.hgym_prof_enable(1), "hgym_prof_enable")
    net.act(obs, priv, z=z, out=out)
    net.act(obs, priv, z=z, out=out)
    assert L.prof_summary(L.PROF_POLICY)[0] == 2
    L.check(L.lib.hgym_prof_enable(1), "hgym_prof_enable")
    assert L.prof_summary(L.PROF_POLICY) == (0, 0.0, 0.0)
    net.act(obs, priv, z=z, out=out)
    assert L.prof_summary(L.PROF_POLICY)[0] == 1
    n, ms, work = C.c_int64(7), C.c_double(7.0), C.c_double(7.0)
    E_BADARG = -1
    for cls in (-1, 12, 1 << 20):
        assert L.lib.hgym_prof_summary(cls, C.byref(n), C.byref(ms), C.byref(work)) == E_BADARG
    assert L.lib.hgym_prof_summary(L.PROF_POLICY, None, C.byref(ms), C.byref(work)) == E_BADARG
    assert L.lib.hgym_prof_summary(L.PROF_POLICY, C.byref(n), None, C.byref(work)) == E_BADARG
    assert L.lib.hgym_prof_summary(L.PROF_POLICY, C.byref(n), C.byref(ms), None) == E_BADARG
    assert (n.value, ms.value, work.value) == (7, 7.0, 7.0), "a refused summary wrote its outputs"
