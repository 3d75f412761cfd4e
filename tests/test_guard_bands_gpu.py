"""-m gpu: every entry point of include/hgym.h stays inside the caller's buffers.  The library never allocates;
every kernel writes through raw pointers whose extents come from the caller's shapes or from the header's size macros, and PyTorch's
caching allocator hides a store a few rows past M in its slack.  Every case here runs the entry point twice on the same inputs --
once on ordinary torch tensors (the twin), once with EVERY pointer argument carved from a tests/guard_common.py Arena at exactly the
stated size -- and asserts
  (a) arena.verify is clean after each call: no byte of any guard band changed;
  (b) every output has the bits of the twin's (the means over resetting envs, which the suite already treats as order-dependent fp32
      atomics -- episode_acc, extras_episode, custom_acc, extras_custom -- are compared as tests/env_common.py compares them);
  (c) every float output is finite: the bands and the input slack the cases poison (rows no index names, columns in [width, ld), rows
      past M of a shadow) are 0xFF = NaN, so a consumed read outside the stated ranges shows.

Detected: every store outside the stated ranges up to BAND (256 KiB) away, and every consumed load.  NOT detected: a load of band
bytes that is masked out afterwards -- at the end of a real allocation it would still be out of bounds; only a sanitizer could see
it, and none may run on the GPU here.

Out of scope: hgym_comm_* (several processes and peer-mapped memory the caller does not carve) and any search of compiled code.
(hgym_prof_*: tests/test_prof_hooks_gpu.py, on this module's helpers.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import guard_common as G
import update_options_common as U
from hgym import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 1e-3
MAX_BATCH = 256
F32, BF16, F64, I64, I32, U8 = torch.float32, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.uint8
ATOMIC = ("episode_acc", "extras_episode", "custom_acc", "extras_custom")      # fp32 atomics in arrival order (tests/env_common.py)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(U8).cpu()


def _all_ff(t):
    return bool((t.contiguous().reshape(-1).view(U8) == 0xFF).all())


class Side:
    """One of the two runs of a case: its allocator (G.Plain for the twin, a G.Arena for the guarded run), its net, and verify()."""

    def __init__(self, what, A, net=None, arenas=()):
        self.what, self.A, self.net, self.arenas = what, A, net, tuple(arenas)

    def verify(self, call):
        torch.cuda.synchronize()
        for a in self.arenas:
            a.verify("%s: %s" % (self.what, call))


def _compare(twin, got, what):
    """(b) and (c).  Keys starting with "raw:" hold bytes that are not floats to be judged (guard bytes the call must leave)."""
    assert list(twin) == list(got)
    for k in twin:
        a, b = twin[k], got[k]
        if k.endswith("grad_sqnorm"):
            _compare_sqnorm(float(a), float(b), "%s: %s" % (what, k))
        elif k.split(".")[-1] in ATOMIC:
            np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg="%s: %s" % (what, k))
        else:
            ab, bb = _bits(a), _bits(b)
            assert torch.equal(ab, bb), "%s: %s differs from the unguarded twin's in %d bytes, first at %d" % (
                what, k, int((ab != bb).sum()), int((ab != bb).nonzero()[0]))
        if b.is_floating_point() and not k.startswith("raw:"):
            assert bool(torch.isfinite(b.float()).all()), "%s: %s is not finite: a guard byte or a poisoned input was consumed" % (what, k)


def _compare_sqnorm(a, b, what):
    """opt_state[HGYM_OPT_GRAD_SQNORM] as hgym_ppo_grad leaves it: one fp64 atomic per workgroup of reduce_slabs_kernel (at most 1 632), every
    partial pre-rounded to 2^-46 -- exact, hence order-independent, additions while the total stays below 2^53 quanta = 128, which the
    kernel's comment promises and this holds to the bit.  Above 128 (a gradient norm beyond 11.3: the one-row minibatches here) the
    additions round and the kernel documents the last bits as order-dependent: 1 632 roundings of 2^-53 relative each, 1.9e-13.  (With
    grad_norm_ready = 0, as every case here runs, hgym_ppo_apply does not read the slot: it forms the norm itself, in a fixed order.)"""
    if a < 128.0 and b < 128.0:
        assert a == b, "%s: %r against the twin's %r" % (what, b, a)
    else:
        assert abs(a - b) <= 1632 * 2.0 ** -53 * abs(a), "%s: %r against the twin's %r" % (what, b, a)


def _opt_state(net, out, tag):
    o = net.opt_state.clone()
    out[tag + ".grad_sqnorm"] = o[L.OPT_GRAD_SQNORM].clone()
    o[L.OPT_GRAD_SQNORM] = 0.0
    out[tag] = o


def _pair(case, what, nbytes=48 << 20, nets=None):
    """case(side) -> {name: output tensor}, run on the twin and on an arena of nbytes; nets: (twin net, guarded net, its arena)."""
    tn, gn, na = nets if nets is not None else (None, None, None)
    twin = case(Side(what, G.Plain(DEV), tn))
    torch.cuda.synchronize()
    arena = G.Arena(DEV, nbytes)
    side = Side(what, arena, gn, (arena,) + ((na,) if na is not None else ()))
    got = case(side)
    side.verify("end of the case")
    _compare(twin, got, what)


# ------------------------------------------------------------------------------------------------ the harness, once, on the device
def test_verify_raises_on_a_device_overrun():
    """Plain torch writes one element past a carved buffer through a wider view of the same allocation: verify must raise, and names it."""
    a = G.Arena(DEV, G.arena_bytes(4096, 4096))
    a.carve(16, F32, name="before")
    x = a.carve((10, 3), F32, name="x")
    x.zero_()
    a.verify("zero fill")
    off = x.data_ptr() - a.raw.data_ptr()
    a.raw[off:off + 4 * 31].view(F32)[30] = 1.0
    torch.cuda.synchronize()
    with pytest.raises(G.GuardError) as e:
        a.verify("torch writer")
    assert "x: behind band, bytes [120, 123] relative to the buffer, 4 changed" in str(e.value) and "before" not in str(e.value)
    a.verify("refilled")
    assert torch.isnan(a.raw[off:off + 4 * 31].view(F32).sum()) and float(x.sum()) == 0.0


# ------------------------------------------------------------------------------------------------ storage side
@pytest.mark.parametrize("boot", [False, True], ids=["gae", "gae_bootstrap"])
@pytest.mark.parametrize("T,N", [(1, 1), (2, 15), (5, 17), (65, 33), (3, 257)])
def test_gae(T, N, boot):
    """stats is exactly HGYM_GAE_STATS_DOUBLES(N) doubles; dones / time_outs are byte arrays (the header asks no alignment of them:
    the kernel reads them byte by byte), carved at an odd address."""
    def case(side):
        A, g = side.A, _gen(100 * T + N)
        rew, val = A.place(torch.randn(T, N, generator=g)), A.place(torch.randn(T, N, generator=g))
        dones = A.place((torch.rand(T, N, generator=g) < 0.2).to(U8), skew=1)
        tos = A.place((torch.rand(T, N, generator=g) < 0.2).to(U8), skew=1)
        last = A.place(torch.randn(N, generator=g))
        ret, adv = A.carve((T, N), F32), A.carve((T, N), F32)
        stats = A.zeros(G.gae_stats_doubles(N), F64)
        for rep in range(2):        # the second call finds the arrival counter the first one left
            if boot:
                L.check(L.lib.hgym_gae_bootstrap(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dones), L.u8ptr(tos), L.fptr(last), 0.99, 0.95,
                                                 L.fptr(ret), L.fptr(adv), L.f64ptr(stats), _s()), "hgym_gae_bootstrap")
            else:
                L.check(L.lib.hgym_gae(T, N, L.fptr(rew), L.fptr(val), L.u8ptr(dones), L.fptr(last), 0.99, 0.95, L.fptr(ret), L.fptr(adv),
                                       L.f64ptr(stats), _s()), "hgym_gae")
            side.verify("call %d" % rep)
        assert float(stats[3]) == 0.0 and float(stats[2]) == T * N
        return dict(returns=ret, advantages=adv, stats=stats, rewards=rew)
    _pair(case, "%s T=%d N=%d" % ("hgym_gae_bootstrap" if boot else "hgym_gae", T, N))


@pytest.mark.parametrize("count", [2, 255, 257, 1025])
def test_adv_normalize(count):
    def case(side):
        A, g = side.A, _gen(count)
        x = torch.randn(count, generator=g)
        adv = A.place(x)
        stats = A.place(torch.tensor([float(x.double().sum()), float((x.double() ** 2).sum()), float(count)], dtype=F64))
        L.check(L.lib.hgym_adv_normalize(count, L.fptr(adv), L.f64ptr(stats), _s()), "hgym_adv_normalize")
        side.verify("the call")
        return dict(advantages=adv, stats=stats)
    _pair(case, "hgym_adv_normalize count=%d" % count)


@pytest.mark.parametrize("segments,seg_len", [(1, 2), (3, 1023), (4, 1025), (7, 43)])
def test_adv_normalize_minibatches(segments, seg_len):
    """rows = segments * seg_len + 5: five rows no entry names; the scratch is exactly the macro's size."""
    n = segments * seg_len
    rows = n + 5

    def case(side):
        A, g = side.A, _gen(n)
        perm = torch.randperm(rows, generator=g)
        idx = A.place(perm[:n].contiguous())
        adv = A.place(torch.randn(rows, generator=g))
        adv[perm[n:].to(DEV)] = float("nan")      # rows no entry names: poisoned
        out = A.carve(rows, F32)
        scratch = A.zeros(G.adv_mb_scratch_doubles(segments, seg_len), F64)
        for rep in range(2):
            L.check(L.lib.hgym_adv_normalize_minibatches(segments, seg_len, L.i64ptr(idx), L.fptr(adv), L.fptr(out), rows, L.f64ptr(scratch),
                                                         _s()), "hgym_adv_normalize_minibatches")
            side.verify("call %d" % rep)
        assert _all_ff(out[perm[n:].to(DEV)]), "a row of `out` that no entry names was written"
        return {"out": out[idx], "raw:out": out, "raw:scratch": scratch}
    _pair(case, "hgym_adv_normalize_minibatches segments=%d seg_len=%d" % (segments, seg_len))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_store_step(n):
    def case(side):
        A, g = side.A, _gen(n)
        rew, val = A.place(torch.randn(n, generator=g)), A.place(torch.randn(n, generator=g))
        tos = A.place((torch.rand(n, generator=g) < 0.3).to(U8), skew=1)
        dones = A.place((torch.rand(n, generator=g) < 0.3).to(U8), skew=1)
        rs, ds = A.carve(n, F32), A.carve(n, U8, skew=1)
        L.check(L.lib.hgym_store_step(n, L.fptr(rew), L.fptr(val), L.u8ptr(tos), L.u8ptr(dones), 0.99, L.fptr(rs), L.u8ptr(ds), _s()),
                "hgym_store_step")
        side.verify("the call")
        return dict(rewards_slot=rs, dones_slot=ds)
    _pair(case, "hgym_store_step n=%d" % n)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 1000, 4097])
def test_randperm(n):
    """The Feistel domain is a power of four >= n and the walk skips what lies outside [0, n): the band behind `out` is the point."""
    def case(side):
        A = side.A
        out, out_dev = A.carve(n, I64), A.carve(n, I64)
        draw = A.place(torch.tensor([3], dtype=I64))
        L.check(L.lib.hgym_randperm(n, 1234, 3, L.i64ptr(out), _s()), "hgym_randperm")
        side.verify("hgym_randperm")
        L.check(L.lib.hgym_randperm_dev(n, 1234, L.i64ptr(draw), L.i64ptr(out_dev), _s()), "hgym_randperm_dev")
        side.verify("hgym_randperm_dev")
        assert torch.equal(out.sort().values, torch.arange(n, device=DEV)) and torch.equal(out, out_dev) and int(draw) == 3
        return dict(out=out, out_dev=out_dev)
    _pair(case, "hgym_randperm n=%d" % n)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("width", [12, 47, 705])
@pytest.mark.parametrize("M", [1, 3, 65])
def test_mirror_rows(M, width, dtype):
    """ld_dst > zero_to > width; columns [zero_to, ld_dst) keep 0xFF; src columns [width, ld_src) are 0xFF; both element-aligned only."""
    es = G.esize(dtype)
    ld_src, zero_to = width + 3, width + 2
    ld_dst = zero_to + 3

    def case(side):
        A, g = side.A, _gen(1000 * M + width)
        src = A.carve((M, ld_src), dtype, skew=es)
        src[:, :width] = torch.randn(M, width, generator=g).to(dtype).to(DEV)
        dst = A.carve((M, ld_dst), dtype, skew=es)
        col = A.place(torch.randperm(width, generator=g).to(I32))
        sign = A.place(torch.where(torch.rand(width, generator=g) < 0.5, -1.0, 1.0).float())
        L.check(L.lib.hgym_mirror_rows(M, width, C.cast(col.data_ptr(), C.POINTER(C.c_int32)), L.fptr(sign), C.c_void_p(src.data_ptr()), ld_src,
                                       C.c_void_p(dst.data_ptr()), ld_dst, zero_to, L.F32 if dtype == F32 else L.BF16, _s()), "hgym_mirror_rows")
        side.verify("the call")
        assert _all_ff(dst[:, zero_to:]), "columns [zero_to, ld_dst) were written"
        assert _all_ff(src[:, width:]) and bool((dst[:, width:zero_to].contiguous().view(torch.int16) == 0).all())
        assert torch.equal(dst[:, :width], src[:, :width][:, col.long()] * sign.to(dtype))
        return {"dst": dst[:, :zero_to], "raw:dst": dst}
    _pair(case, "hgym_mirror_rows M=%d width=%d %s" % (M, width, dtype))


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_eval_accumulate(n):
    def case(side):
        A, g = side.A, _gen(n)
        block = A.carve(G.eval_block_doubles(n), F64)
        L.check(L.lib.hgym_eval_reset(n, L.f64ptr(block), _s()), "hgym_eval_reset")
        side.verify("hgym_eval_reset")
        for t in range(3):
            f = [A.place(torch.randn(c, n, generator=g)) for c in (4, 3, 3, L.NUM_REWARDS)]
            rew = A.place(torch.randn(n, generator=g))
            reset = A.place((torch.rand(n, generator=g) < 0.3).to(U8), skew=1)
            tout = A.place(((torch.rand(n, generator=g) < 0.5).to(U8) * reset.cpu()), skew=1)
            L.check(L.lib.hgym_eval_accumulate(n, L.fptr(f[0]), L.fptr(f[1]), L.fptr(f[2]), L.fptr(f[3]), L.fptr(rew), L.u8ptr(reset), L.u8ptr(tout),
                                               L.f64ptr(block), _s()), "hgym_eval_accumulate")
            side.verify("hgym_eval_accumulate %d" % t)
        assert float(block[L.EVAL_STEPS]) == 3.0 and float(block[L.EVAL_ENV_STEPS]) == 3.0 * n
        return dict(block=block)
    _pair(case, "hgym_eval_reset + hgym_eval_accumulate n=%d" % n)


# ------------------------------------------------------------------------------------------------ nets
# (path, auxiliary head): the three of update_options_common.SHAPES, max_batch = 256; the fused net with and without the head
NET_IDS = [("bf16-fused", True), ("bf16-fused", False), ("f32-layer", False), ("bf16-layer", False)]
NET_NAMES = ["%s%s" % (p, "-aux" if a else "") for p, a in NET_IDS]
_NETS, _CASES = {}, {}


def _opts(path, aux=False, std="scalar", norm=False, unclipped=False, act=None):
    """act: None (ELU(1)) or update_options_common.TANH, which the fused kernels run through their any-activation instantiations."""
    return U.Options(path, act, std, unclipped, aux, norm, False)


def _case(opts, B=97):
    key = (opts, B)
    if key not in _CASES:
        _CASES[key] = U.make_case(opts, S=130, B=B, seed=len(_CASES))
    return _CASES[key]


def _nets(opts, net=None, max_batch=MAX_BATCH):
    """(twin, guarded net, the guarded net's arena) per configuration; the guarded net's buffers have exactly the header's sizes.
    net: (num_obs, num_priv, num_actions, actor hidden, critic hidden) instead of the path's own shape.  max_batch: for the fused rollout
    at more than 256 envs (a launch is one batch of num_envs rows)."""
    from hgym import NetBuffers, make_net_config, norm_layout
    key = (opts.path, opts.aux, opts.std, opts.norm, str(net), opts.activation is not None, max_batch)
    if key not in _NETS:
        sh = U.SHAPES[opts.path]
        no, npv, A, ah, ch = net or sh["net"]
        kw = dict(aux_hidden=sh["aux"][0], aux_out=sh["aux"][1], aux_target_offset=sh["aux"][2]) if opts.aux else {}
        cfg = make_net_config(no, npv, A, ah, ch, "f32" if opts.path == "f32-layer" else "bf16", max_batch,
                              fused_activation=opts.path == "bf16-fused", noise_std_type=opts.std, activation=opts.activation, **kw)
        on = (U.EPS, None) if opts.norm else None
        twin = NetBuffers(cfg, DEV, learning_rate=LR, obs_norm=on)
        arena = G.Arena(DEV, G.net_arena_bytes(cfg, opts.norm))
        net = G.guard_net(cfg, arena, learning_rate=LR, obs_norm=on)
        torch.cuda.synchronize()
        arena.verify("hgym_net_norm_init %s" % (key,))
        assert net.workspace.numel() == int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) and net._ws_ptr % 256 == 0
        assert net.grads_ext.numel() == net.P + 1 and net.params.numel() == net.P and net.opt_state.numel() == L.OPT_STATE
        if opts.norm:
            assert net._norm_block.numel() == norm_layout(cfg)[L.NORM_BYTES] and net._norm_block.data_ptr() % 256 == 0
        assert (net.shadow_ld(0) > 0) == (opts.path == "bf16-fused")
        _NETS[key] = (twin, net, arena)
    return _NETS[key]


def _fresh(net, opts, case):
    """Back to the case's parameters and statistics from a zero-filled workspace and optimiser: both nets of a pair start a case alike."""
    for t in (net.adam_m, net.adam_v, net.grads_ext, net.opt_state, net.workspace):
        t.zero_()
    net.opt_state[L.OPT_LR] = LR
    net.load_state_dict(case["params"])
    if opts.norm:
        net.load_norm_state(U.norm_state_of(case["stats"]))
        net.sync_shadow()


def _dims(opts):
    no, npv, A = U.SHAPES[opts.path]["net"][:3]
    return no, npv, A


def _shadows(side, M, extra=3):
    """(obs_bf16, priv_bf16) of M + extra rows, or (None, None) off the fused path: rows >= M must keep their guard bytes."""
    ld = side.net.shadow_ld(0), side.net.shadow_ld(1)
    if ld[0] == 0:
        return None, None
    return side.A.carve((M + extra, ld[0]), BF16), side.A.carve((M + extra, ld[1]), BF16)


def _check_shadow(sh, M, width, what):
    assert _all_ff(sh[M:]), "%s: shadow rows >= M were written" % what
    assert bool((sh[:M, width:].contiguous().view(torch.int16) == 0).all()), "%s: shadow pad columns are not zero" % what


def _act(side, M, obs, priv, z, shadow, out, tag):
    """hgym_policy_act into carved outputs; z None: Philox keyed by a carved step counter."""
    A_, net = side.A, side.net
    A = net.cfg.num_actions
    o = dict(actions=A_.carve((M, A), F32), mu=A_.carve((M, A), F32), sigma=A_.carve((M, A), F32), logp=A_.carve(M, F32), values=A_.carve(M, F32))
    step = A_.place(torch.tensor([5], dtype=I64))
    sh = None if shadow is None else C.byref(net.shadow_struct(*shadow))
    L.check(L.lib.hgym_policy_act(C.byref(net.cfg), C.byref(net.struct), M, L.fptr(obs), L.fptr(priv), L.fptr(z), 77, L.i64ptr(step),
                                  L.fptr(o["actions"]), L.fptr(o["mu"]), L.fptr(o["sigma"]), L.fptr(o["logp"]), L.fptr(o["values"]), sh, _s()),
            "hgym_policy_act")
    side.verify("hgym_policy_act %s" % tag)
    for k, v in o.items():
        out["%s.%s" % (tag, k)] = v
    if shadow is not None:
        _check_shadow(shadow[0], M, net.cfg.num_obs, tag)
        _check_shadow(shadow[1], M, net.cfg.num_priv, tag)
        out["%s.obs_bf16" % tag], out["%s.priv_bf16" % tag] = shadow[0][:M], shadow[1][:M]


MS = [1, 31, 33, 63, 65, 97]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("path,aux", NET_IDS, ids=NET_NAMES)
def test_mlp_forward(path, aux, M):
    """x with ldx = in + 3 and a NaN tail in every row, carved at skew 4 (rows of 705 floats are never 16-byte aligned in the storage);
    y at skew 0 and 4; which 0, 1, and 2 with the head."""
    opts = _opts(path, aux)
    case = _case(opts)
    dims = _dims(opts)

    def run(side):
        net, A, out, g = side.net, side.A, {}, _gen(M)
        _fresh(net, opts, case)
        for which in (0, 1) + ((2,) if aux else ()):
            nin = (dims[0], dims[1], dims[0])[which]
            nout = (dims[2], 1, U.SHAPES[path]["aux"][1])[which]
            x = A.carve((M, nin + 3), F32, skew=4)
            x[:, :nin] = torch.randn(M, nin, generator=g).to(DEV)
            for skew in (0, 4):
                y = A.carve((M, nout), F32, skew=skew)
                L.check(L.lib.hgym_mlp_forward(C.byref(net.cfg), C.byref(net.struct), which, M, L.fptr(x), nin + 3, L.fptr(y), _s()), "hgym_mlp_forward")
                side.verify("which=%d M=%d y skew %d" % (which, M, skew))
                out["y%d.skew%d" % (which, skew)] = y
            assert _all_ff(x[:, nin:])
        return out
    _pair(run, "hgym_mlp_forward %s M=%d" % (path, M), nets=_nets(opts))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("path,aux", NET_IDS, ids=NET_NAMES)
def test_policy_act(path, aux, M):
    """z given and z = NULL, with and without HgymObsShadow (the fused path): shadow rows [0, M) have zero pad columns, rows >= M keep
    their guard bytes."""
    opts = _opts(path, aux)
    case = _case(opts)
    no, npv, A = _dims(opts)

    def run(side):
        net, out, g = side.net, {}, _gen(M + 1)
        _fresh(net, opts, case)
        obs, priv = side.A.place(torch.randn(M, no, generator=g), skew=4), side.A.place(torch.randn(M, npv, generator=g), skew=4)
        z = side.A.place(torch.randn(M, A, generator=g))
        for zt, zn in ((z, "z"), (None, "philox")):
            for with_shadow in ((False, True) if net.shadow_ld(0) else (False,)):
                _act(side, M, obs, priv, zt, _shadows(side, M) if with_shadow else None, out, "%s%s" % (zn, "+shadow" if with_shadow else ""))
        return out
    _pair(run, "hgym_policy_act %s M=%d" % (path, M), nets=_nets(opts))


@pytest.mark.parametrize("M", [1, 255, 257, 513])
@pytest.mark.parametrize("path,aux", NET_IDS[1:], ids=NET_NAMES[1:])
def test_critic_values(path, aux, M):
    """M crosses max_batch = 256 in pieces; with and without the shadow."""
    opts = _opts(path, aux)
    case = _case(opts)
    no, npv, A = _dims(opts)

    def run(side):
        net, out, g = side.net, {}, _gen(M + 2)
        _fresh(net, opts, case)
        priv = side.A.place(torch.randn(M, npv, generator=g), skew=4)
        for with_shadow in ((False, True) if net.shadow_ld(1) else (False,)):
            v = side.A.carve(M, F32)
            sp = side.A.carve((M + 2, net.shadow_ld(1)), BF16) if with_shadow else None
            sh = C.byref(net.shadow_struct(None, sp)) if with_shadow else None
            L.check(L.lib.hgym_critic_values(C.byref(net.cfg), C.byref(net.struct), M, L.fptr(priv), L.fptr(v), sh, _s()), "hgym_critic_values")
            side.verify("shadow %s" % with_shadow)
            out["values.shadow%d" % with_shadow] = v
            if with_shadow:
                _check_shadow(sp, M, npv, "hgym_critic_values")
                out["priv_bf16"] = sp[:M]
        return out
    _pair(run, "hgym_critic_values %s M=%d" % (path, M), nets=_nets(opts))


# hgym_ppo_grad: (path, B, variant).  Every path: the three B on fp32 rows, then one case each with the mirror loss, log std, the
# normaliser, the unclipped value loss and the two-part call; the fused path again from bf16 shadows (and the mirror loss from them).
GRAD_CASES = []
for _p in U.PATHS:
    GRAD_CASES += [(_p, b, "rows") for b in (1, 33, 97)]
    if _p == "bf16-fused":
        GRAD_CASES += [(_p, b, "shadow") for b in (1, 33, 97)] + [(_p, 97, "shadow+mirror"), (_p, 97, "aux")]
    GRAD_CASES += [(_p, 97, v) for v in ("mirror", "log", "norm", "unclipped")] + [(_p, 33, "part")]


@pytest.mark.parametrize("path,B,variant", GRAD_CASES, ids=["%s-B%d-%s" % c for c in GRAD_CASES])
def test_ppo_update(path, B, variant):
    """hgym_ppo_grad (or hgym_ppo_grad_part 0, 1) on S = 130 stored rows of which idx names B -- every other row of the nine columns and
    of the shadows is 0xFF --, then hgym_net_norm_unfold_grad, hgym_ppo_apply and, WITHOUT hgym_net_sync_shadow, one hgym_policy_act (a
    corrupted operand copy shows up there).  verify after each call: the workspace and grads_ext bands are the point.  With the mirror
    loss mirror_target is exactly (B, A), mirror_sums 2 doubles, pair_idx exactly B."""
    from hgym import make_batch, make_ppo_config
    opts = _opts(path, aux=variant == "aux", std="log" if variant == "log" else "scalar", norm=variant == "norm", unclipped=variant == "unclipped")
    case = _case(opts, B)
    no, npv, A = _dims(opts)
    S, mirror, shadow = case["S"], "mirror" in variant, "shadow" in variant
    idx_h = case["idx"]
    pair_h = idx_h.roll(1).contiguous()
    unnamed = torch.ones(S, dtype=torch.bool)
    unnamed[idx_h] = False

    def poison(t):
        t.view(U8).view(S, -1)[unnamed.to(DEV)] = 0xFF

    def run(side):
        net, A_, out, g = side.net, side.A, {}, _gen(B)
        _fresh(net, opts, case)
        cols = [A_.place(t, skew=4 if i < 2 else 0) for i, t in enumerate(case["cols"])]
        kw = {}
        if shadow:
            sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(BF16)
            kw.update(obs_bf16=A_.place(sh(case["cols"][0], net.shadow_ld(0))), priv_bf16=A_.place(sh(case["cols"][1], net.shadow_ld(1))))
        for t in cols + list(kw.values()):
            poison(t)
        idx = A_.place(idx_h)
        if mirror:
            src = A_.place(torch.randperm(A, generator=g).to(I32))
            sign = A_.place(torch.where(torch.rand(A, generator=g) < 0.5, -1.0, 1.0).float())
            target, sums = A_.carve((B, A), F32), A_.zeros(2, F64)
            kw.update(pair_idx=A_.place(pair_h), mirror=(src, sign, target, sums))
        ppo = make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"], clipped_value_loss=not opts.unclipped,
                              mirror_coef=0.5 if mirror else 0.0)
        batch = make_batch(*cols, idx, **kw)
        if variant == "part":
            for part in (0, 1):
                net.ppo_grad_part(ppo, batch, part)
                side.verify("hgym_ppo_grad_part %d" % part)
        else:
            net.ppo_grad(ppo, batch)
            side.verify("hgym_ppo_grad")
        out["grads_ext"] = net.grads_ext.clone()
        _opt_state(net, out, "opt_state after grad")
        if mirror:
            out["mirror_target"], out["mirror_sums"] = target, sums
            assert float(sums[1]) == 1.0
        if opts.norm:
            net.norm_unfold_grad()
            side.verify("hgym_net_norm_unfold_grad")
            out["grads_ext unfolded"] = net.grads_ext.clone()
        net.ppo_apply(ppo)
        side.verify("hgym_ppo_apply")
        out.update(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone(), sigma=net.sigma.clone())
        _opt_state(net, out, "opt_state")
        M = 33
        obs, priv = A_.place(case["cols"][0][:M].contiguous(), skew=4), A_.place(case["cols"][1][:M].contiguous(), skew=4)
        _act(side, M, obs, priv, A_.place(torch.randn(M, A, generator=g)), None, out, "act after the step")
        return out
    _pair(run, "PPO update %s B=%d %s" % (path, B, variant), nets=_nets(opts))


@pytest.mark.parametrize("path", U.PATHS)
def test_obs_norm(path):
    """hgym_net_norm_init, _accumulate, _merge and hgym_net_sync_shadow at M = 1, rows_per_wg - 1, rows_per_wg + 1 and
    2 * rows_per_wg * wgs + 1 (hgym_net_norm_layout), obs and priv carved at skew 4 and at skew 0 (the 16-byte fast path)."""
    from hgym import norm_layout
    opts = _opts(path, norm=True)
    case = _case(opts)
    no, npv, A = _dims(opts)
    nets = _nets(opts)
    lay = norm_layout(nets[0].cfg)
    rpw, wgs = int(lay[L.NORM_ROWS_PER_WG]), max(int(lay[L.NORM_WGS]), int(lay[L.NORM_WGS + 1]))
    for M in (1, rpw - 1, rpw + 1, 2 * rpw * wgs + 1):
        def run(side):
            net, out = side.net, {}
            _fresh(net, opts, case)
            L.check(L.lib.hgym_net_norm_init(C.byref(net.cfg), C.byref(net.struct), U.EPS, -1, _s()), "hgym_net_norm_init")
            side.verify("hgym_net_norm_init")
            net.sync_shadow()
            side.verify("hgym_net_sync_shadow after init")
            for skew in (4, 0):
                g = torch.Generator(device=DEV).manual_seed(M + skew)
                obs, priv = side.A.carve((M, no), F32, skew=skew), side.A.carve((M, npv), F32, skew=skew)
                obs.copy_(torch.randn(M, no, device=DEV, generator=g) * 2.0 + 0.5)
                priv.copy_(torch.randn(M, npv, device=DEV, generator=g) * 0.5 - 1.0)
                net.norm_accumulate(obs, priv)
                side.verify("hgym_net_norm_accumulate M=%d skew %d" % (M, skew))
                out["sums.skew%d" % skew] = net.norm_view("sums").clone()
                net.norm_merge()
                side.verify("hgym_net_norm_merge M=%d skew %d" % (M, skew))
                net.sync_shadow()
                side.verify("hgym_net_sync_shadow M=%d skew %d" % (M, skew))
                for k in (0, 1):
                    for name in ("mean", "var", "mean_f", "scale_f", "bias"):
                        out["%s%d.skew%d" % (name, k, skew)] = net.norm_view(name, k).clone()
                assert float(out["sums.skew%d" % skew][0]) == M
            x = side.A.place(torch.randn(5, no, generator=_gen(M)), skew=4)
            y = side.A.carve((5, A), F32)
            L.check(L.lib.hgym_mlp_forward(C.byref(net.cfg), C.byref(net.struct), 0, 5, L.fptr(x), no, L.fptr(y), _s()), "hgym_mlp_forward")
            side.verify("hgym_mlp_forward on the refolded net")
            out["mu"] = y
            return out
        _pair(run, "observation normaliser %s M=%d" % (path, M), nbytes=G.arena_bytes(*[4 * M * k for k in (no, npv, no, npv)], *[1 << 20] * 4), nets=nets)


@pytest.mark.parametrize("M", [1, 255, 257, 513])
@pytest.mark.parametrize("path", U.PATHS)
def test_ppo_diagnostics(path, M):
    """hgym_ppo_diag_reset + hgym_ppo_diagnostics, then hgym_ppo_diag_reduce in two pieces: the block is exactly
    HGYM_DIAG_BLOCK_DOUBLES(M) doubles, the scratch exactly max_batch x 13 floats, every column exactly M rows."""
    from hgym import make_ppo_config
    opts = _opts(path)
    if path == "f32-layer":
        # the reduction reads 12-wide action rows (HGYM_E_UNSUPPORTED otherwise): the path's ragged widths with 12 actions
        no, npv, A = 37, 19, 12
        nets = _nets(opts, net=(no, npv, A, [24, 16], [24, 16]))
        g0 = _gen(12)
        case = dict(params={k: (0.5 + torch.rand(v.shape, generator=g0)) if k == "std" else 0.2 * torch.randn(v.shape, generator=g0)
                            for k, v in nets[0].views.items()})
    else:
        (no, npv, A), case, nets = _dims(opts), _case(opts), _nets(opts)

    def run(side):
        net, A_, g = side.net, side.A, _gen(M + 3)
        _fresh(net, opts, case)
        r = lambda *s: torch.randn(*s, generator=g)
        # obs, priv, actions, values, advantages, returns, logp, mu, sigma
        cols = [A_.place(r(M, no), skew=4), A_.place(r(M, npv), skew=4), A_.place(r(M, A)), A_.place(r(M)), A_.place(r(M)), A_.place(r(M)),
                A_.place(-10.0 + r(M)), A_.place(r(M, A)), A_.place(0.5 + torch.rand(M, A, generator=g))]
        block, scratch = A_.carve(G.diag_block_doubles(M), F64), A_.carve(MAX_BATCH * 13, F32)
        ppo = make_ppo_config()
        rows = L.Batch(*[L.fptr(t) for t in cols], None, 0, None, None, M)
        L.check(L.lib.hgym_ppo_diag_reset(M, L.f64ptr(block), _s()), "hgym_ppo_diag_reset")
        side.verify("hgym_ppo_diag_reset")
        L.check(L.lib.hgym_ppo_diagnostics(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(rows), M, L.fptr(scratch), L.f64ptr(block),
                                           _s()), "hgym_ppo_diagnostics")
        side.verify("hgym_ppo_diagnostics")
        assert float(block[L.DIAG_COUNT]) == M
        # the reduction alone, in two pieces, on columns of the caller: mu_new / values_new exactly M rows, std exactly A floats
        block2 = A_.carve(G.diag_block_doubles(M), F64)
        mu_new, v_new, std = A_.place(r(M, A)), A_.place(r(M)), A_.place(0.5 + torch.rand(A, generator=g))
        L.check(L.lib.hgym_ppo_diag_reset(M, L.f64ptr(block2), _s()), "hgym_ppo_diag_reset")
        # (a piece that is not the last must be a multiple of 256 rows: below 257 rows the second, finishing piece holds all of them)
        cut = 256 if M > 256 else 0
        for m0, m1, fin in ((0, cut, 0), (cut, M, 1))[0 if cut else 1:]:
            # actions, mu_old, sigma_old, mu_new, logp_old, values_old, returns, advantages, values_new
            p = [L.fptr(t[m0:m1]) if m1 > m0 else None for t in (cols[2], cols[7], cols[8], mu_new, cols[6], cols[3], cols[5], cols[4], v_new)]
            L.check(L.lib.hgym_ppo_diag_reduce(m1 - m0, *p, L.fptr(std), 0.2, m0, M, fin, L.f64ptr(block2), _s()), "hgym_ppo_diag_reduce")
            side.verify("hgym_ppo_diag_reduce rows [%d, %d)" % (m0, m1))
        assert float(block2[L.DIAG_COUNT]) == M
        return dict(block=block, block2=block2)
    _pair(run, "diagnostics %s M=%d" % (path, M), nets=nets)


# ------------------------------------------------------------------------------------------------ env side
def _plant(buf, N):
    """Time-outs, a command resample and a push inside three steps, as tests/env_common.py::run_random_trace plants them."""
    ep = (torch.arange(N) * 37) % 2390
    ep[:min(N, 6)] = torch.tensor([2399, 2398, 799, 1598, 0, 2396])[:min(N, 6)]
    buf.episode_length.copy_(ep)
    buf.counters[L.CNT_STEP] = 397


def _env_state(buf, out, tag=""):
    for name, t, _ in buf.state_entries():
        if t is not None:
            out[tag + name] = t.clone()
    # log_stats[TERMS] sums extras["episode"] over the steps: the same order-dependent means, compared like them
    out[tag + "log_cur"], out[tag + "log_stats"] = buf.log_cur.clone(), buf.log_stats[L.LOG_STEPS:].clone()
    out[tag + "log_stats.extras_episode"] = buf.log_stats[L.LOG_TERMS:L.LOG_STEPS].clone()
    return out


def _make_env(side, N, layout, setup=None, seed=11):
    """EnvBuffers on the side's allocator; the guarded one has every own allocation re-seated before the first struct is built."""
    from hgym import EnvBuffers, default_env_config
    cfg = default_env_config(N, seed=seed)
    buf = EnvBuffers(cfg, DEV, sim_layout=layout)
    buf.log_sink = True
    if setup is not None:
        setup(buf)
    if isinstance(side.A, G.Arena):
        arena = G.Arena(DEV, G.env_arena_bytes(buf))
        G.guard_env(buf, arena)
        assert buf.rollout_scratch.numel() == G.rollout_scratch_bytes(N) and tuple(buf._l0_partial.shape) == (2, N, 512)
        assert buf.f["env_origins"].data_ptr() == buf._state.data_ptr() + 4 * N * (buf._state.shape[0] - 3)
        side.arenas += (arena,)
    return cfg, buf


ENVS = [(37, "soa"), (97, "soa"), (264, "soa"), (97, "aos")]


@pytest.mark.parametrize("N,layout", ENVS, ids=["N%d-%s" % e for e in ENVS])
def test_env_step_calls(N, layout):
    """hgym_env_reset_all, three hgym_env_step_synth, one step as hgym_pre_physics / hgym_pd_torques / hgym_synth_physics /
    hgym_post_physics, a deferred step flushed by hgym_env_finalize, one flushed by hgym_policy_act_fin
    (N <= max_batch) with a transition sink, and hgym_env_reset_idx with 5 ids, on a guarded EnvBuffers: the state has the twin's bits."""
    opts = _opts("bf16-fused")
    case = _case(opts)
    nets = _nets(opts)

    def run(side):
        cfg, buf = _make_env(side, N, layout)
        A_, out, g = side.A, {}, _gen(N)
        sim, st, o = buf.sim_struct(), buf.state_struct(), buf.out_struct()
        nz = buf.noise_struct()
        L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), _s()), "hgym_env_prime")
        side.verify("hgym_env_prime")
        _plant(buf, N)
        L.check(L.lib.hgym_env_reset_all(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), _s()), "hgym_env_reset_all")
        side.verify("hgym_env_reset_all")
        _env_state(buf, out, "reset_all.")
        _plant(buf, N)
        resets = 0
        for t in range(3):
            a = A_.place(torch.randn(N, 12, generator=g) * 1.5)
            L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), L.fptr(a), _s()), "hgym_env_step_synth")
            side.verify("hgym_env_step_synth %d" % t)
            resets += int(buf.time_out.sum())
        assert int(buf.counters[L.CNT_STEP]) == 400 and resets > 0, "the planted time-outs did not happen"
        _env_state(buf, out, "steps.")
        # the same step as its four component launches
        a = A_.place(torch.randn(N, 12, generator=g) * 1.5)
        L.check(L.lib.hgym_pre_physics(C.byref(cfg), C.byref(st), L.fptr(a), C.byref(nz), _s()), "hgym_pre_physics")
        side.verify("hgym_pre_physics")
        L.check(L.lib.hgym_pd_torques(C.byref(cfg), C.byref(sim), C.byref(st), _s()), "hgym_pd_torques")
        side.verify("hgym_pd_torques")
        L.check(L.lib.hgym_synth_physics(C.byref(cfg), C.byref(sim), C.byref(st), _s()), "hgym_synth_physics")
        side.verify("hgym_synth_physics")
        L.check(L.lib.hgym_post_physics(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), _s()), "hgym_post_physics")
        side.verify("hgym_post_physics")
        _env_state(buf, out, "components.")
        # deferred finalisers, with a transition sink of exactly (N,) columns
        buf.episode_length[:3] = 2399
        sink = dict(values=A_.place(torch.randn(N, generator=g)), rewards=A_.carve(N, F32), dones=A_.carve(N, U8, skew=1),
                    step=A_.place(torch.tensor([0], dtype=I64)), gamma=0.99)
        od = buf.out_struct(sink=sink, defer_finalize=True)
        a = A_.place(torch.randn(N, 12, generator=g))
        L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(od), L.fptr(a), _s()), "hgym_env_step_synth")
        side.verify("hgym_env_step_synth, finaliser deferred")
        L.check(L.lib.hgym_env_finalize(C.byref(cfg), C.byref(st), C.byref(od), _s()), "hgym_env_finalize")
        side.verify("hgym_env_finalize")
        out["sink.rewards"], out["sink.dones"] = sink["rewards"].clone(), sink["dones"].clone()
        if N <= MAX_BATCH:
            net = side.net
            _fresh(net, opts, case)
            buf.episode_length[3:5] = 2399
            L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(od), L.fptr(a), _s()), "hgym_env_step_synth")
            side.verify("hgym_env_step_synth, finaliser deferred (2)")
            A = net.cfg.num_actions
            po = dict(actions=A_.carve((N, A), F32), mu=A_.carve((N, A), F32), sigma=A_.carve((N, A), F32), logp=A_.carve(N, F32),
                      values=A_.carve(N, F32))
            z = A_.place(torch.randn(N, A, generator=g))
            L.check(L.lib.hgym_policy_act_fin(C.byref(net.cfg), C.byref(net.struct), N, L.fptr(buf.obs), L.fptr(buf.priv_obs), L.fptr(z), 3, None,
                                              L.fptr(po["actions"]), L.fptr(po["mu"]), L.fptr(po["sigma"]), L.fptr(po["logp"]), L.fptr(po["values"]),
                                              C.byref(cfg), C.byref(st), C.byref(od), None, _s()), "hgym_policy_act_fin")
            side.verify("hgym_policy_act_fin")
            out.update({"act_fin." + k: v for k, v in po.items()})
            out["sink2.rewards"], out["sink2.dones"], out["sink.step"] = sink["rewards"].clone(), sink["dones"].clone(), sink["step"].clone()
        _env_state(buf, out, "deferred.")
        ids = A_.place(torch.tensor([0, N - 1, -2, N // 2, 3], dtype=I64))
        L.check(L.lib.hgym_env_reset_idx(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), L.i64ptr(ids), 5,
                                         L.u8ptr(buf.reset_idx_mask), L.i64ptr(buf.reset_idx_rejected), _s()), "hgym_env_reset_idx")
        side.verify("hgym_env_reset_idx")
        assert int(buf.reset_idx_rejected) == 0 and int(buf.reset_idx_mask.sum()) == 5
        out["reset_idx.mask"] = buf.reset_idx_mask.clone()
        return _env_state(buf, out, "reset_idx.")
    _pair(run, "env step calls N=%d %s" % (N, layout), nets=nets)


@pytest.mark.parametrize("N,layout", ENVS, ids=["N%d-%s" % e for e in ENVS])
def test_env_split_step_and_heights(N, layout):
    """hgym_env_step_begin / hgym_env_step_end with two user-defined terms (one summed in order, one after the clip) on a small terrain
    with height measurements, three steps, then hgym_measure_heights on its own."""
    import env_common as EC

    def setup(buf):
        spec = EC.random_terrain_spec(_gen(N + 7), N, rows=3, cols=2, points=(5, 3))
        buf.set_terrain(spec.origins, spec.levels, spec.types, spec.env_length, spec.curriculum, height_samples=spec.height_samples,
                        height_points=spec.height_points, border_size=spec.border_size, horizontal_scale=spec.hscale, vertical_scale=spec.vscale)
        buf.set_custom_rewards([0, L.NUM_REWARDS + 1])

    def run(side):
        cfg, buf = _make_env(side, N, layout, setup)
        A_, out, g = side.A, {}, _gen(N + 1)
        sim, st, o = buf.sim_struct(), buf.state_struct(), buf.out_struct()
        nz = buf.noise_struct()
        L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), _s()), "hgym_env_prime")
        side.verify("hgym_env_prime")
        _plant(buf, N)
        resets = 0
        for t in range(3):
            a = A_.place(torch.randn(N, 12, generator=g) * 1.5)
            L.check(L.lib.hgym_env_step_begin(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), L.fptr(a), _s()), "hgym_env_step_begin")
            side.verify("hgym_env_step_begin %d" % t)
            buf.custom_rew.copy_(0.01 * torch.randn(2, N, generator=g))
            L.check(L.lib.hgym_env_step_end(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(nz), _s()), "hgym_env_step_end")
            side.verify("hgym_env_step_end %d" % t)
            resets += int(buf.time_out.sum())
        assert int(buf.counters[L.CNT_STEP]) == 400 and resets > 0, "the planted time-outs did not happen"
        _env_state(buf, out, "steps.")
        buf.measured_heights.view(U8).fill_(0xFF)
        L.check(L.lib.hgym_measure_heights(C.byref(cfg), C.byref(st), _s()), "hgym_measure_heights")
        side.verify("hgym_measure_heights")
        out["measured_heights"], out["height_pose"] = buf.measured_heights.clone(), buf.height_pose.clone()
        return out
    _pair(run, "split step + heights N=%d %s" % (N, layout))


def _direct(name, i, call):
    call()


def _rollout_sequence(side, N, T, deferred, opts, case, watch=_direct, info=None, warm=0):
    """T steps of hgym_rollout_begin / _step / _end as rollout_plan(T, deferred, rows ahead, carried first layer, shadows) lays them out
    -- with the critic's tiles inline, or in the values = NULL form followed by hgym_critic_values over every slot -- and one
    hgym_rollout_eval_step.  The storage slots of obs / priv / the shadows and of every per-step column are carved ONE SLOT AT A TIME, with
    bands between them: a write past row N of slot t cannot hide in slot t + 1.  l0_ahead is exactly (2, N, 512), the scratch exactly
    HGYM_ROLLOUT_SCRATCH_BYTES(N).  watch(name, i, call) runs every hgym_rollout_step / hgym_rollout_eval_step launch (tests/test_prof_hooks_gpu.py
    times them and reads the phase buffer in between); info receives the plan and the EnvBuffers.  warm: hgym_env_step_synth steps into slot 0
    ahead of the rollout -- after hgym_env_prime the frame history is zero, and with it every first-layer sum a launch carries ahead (columns
    [47, 47 + 32 kb0) of its rows: the frames of 15 steps ago and later); 15 steps fill the stack."""
    from humanoid.envs.base.legged_robot import rollout_plan
    no, npv, A = _dims(opts)
    net, A_, out = side.net, side.A, {}
    _fresh(net, opts, case)
    cfg, buf = _make_env(side, N, "soa")
    ld = net.shadow_ld(0), net.shadow_ld(1)
    slots = lambda n, shape, dt, **kw: [A_.carve(shape, dt, **kw) for _ in range(n)]
    c = dict(obs=slots(T + 1, (N, no), F32), priv=slots(T + 1, (N, npv), F32), obs_bf16=slots(T, (N, ld[0]), BF16),
             priv_bf16=slots(T, (N, ld[1]), BF16), actions=slots(T, (N, A), F32), mu=slots(T, (N, A), F32), sigma=slots(T, (N, A), F32),
             logp=slots(T, N, F32), values=slots(T, N, F32), rewards=slots(T, N, F32), dones=slots(T, N, U8, skew=1),
             time_outs=slots(T, N, U8, skew=1))
    step = A_.place(torch.tensor([0], dtype=I64))
    sim, st = buf.sim_struct(), buf.state_struct()
    nz = buf.noise_struct()
    o0 = buf.out_struct(c["obs"][0], c["priv"][0])
    L.check(L.lib.hgym_env_prime(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o0), C.byref(nz), _s()), "hgym_env_prime")
    side.verify("hgym_env_prime into slot 0")
    if warm:
        g, wa = _gen(N + warm), A_.carve((N, A), F32)
        for t in range(warm):
            wa.copy_(torch.randn(N, A, generator=g))
            L.check(L.lib.hgym_env_step_synth(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o0), L.fptr(wa), _s()), "hgym_env_step_synth")
        side.verify("%d warm-up steps into slot 0" % warm)
        assert bool((c["obs"][0][:, :47] != 0).any()), "the oldest frame of slot 0 is still zero"
    _plant(buf, N)
    scratch = C.c_void_p(buf.rollout_scratch.data_ptr())
    plan = rollout_plan(T, deferred, True, True, True)
    if info is not None:
        info.update(plan=plan, buf=buf)
    L.check(L.lib.hgym_rollout_begin(C.byref(st), L.i64ptr(step), scratch, (T - 1) & 1, _s()), "hgym_rollout_begin")
    side.verify("hgym_rollout_begin")
    prev = None
    l0 = lambda k: None if k is None else L.fptr(buf.l0_partial(k))
    for i, p in enumerate(plan):
        vals = None if deferred else c["values"][i]
        sink = dict(values=vals, rewards=c["rewards"][i], dones=c["dones"][i], time_outs=c["time_outs"][i] if deferred else None, step=step,
                    gamma=0.99)
        o = buf.out_struct(c["obs"][i + 1], c["priv"][i + 1], sink, True, alt=bool(p.parity))
        o.obs_older_ready, o.l0_ready, o.l0_ahead = int(p.obs_older_ready), l0(p.l0_ready), l0(p.l0_ahead)
        if p.ahead is not None:
            o.obs_ahead, o.priv_ahead = L.fptr(c["obs"][p.ahead]), L.fptr(c["priv"][p.ahead])
        if p.bf16_ahead:
            o.obs_bf16_ahead, o.ld_obs_bf16_ahead = C.c_void_p(c["obs_bf16"][i + 1].data_ptr()), ld[0]
        sh = net.shadow_struct(c["obs_bf16"][i], c["priv_bf16"][i] if p.shadow_priv else None) if p.shadow_obs else None
        watch("hgym_rollout_step", i, lambda: L.check(L.lib.hgym_rollout_step(
            C.byref(net.cfg), C.byref(net.struct), C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), C.byref(prev) if p.prev else None,
            L.fptr(c["obs"][i]), L.fptr(c["priv"][i]), 99, L.fptr(c["actions"][i]), L.fptr(c["mu"][i]), L.fptr(c["sigma"][i]),
            L.fptr(c["logp"][i]), L.fptr(vals), scratch, p.parity, None if sh is None else C.byref(sh), _s()), "hgym_rollout_step"))
        side.verify("hgym_rollout_step %d" % i)
        prev = o
    L.check(L.lib.hgym_rollout_end(C.byref(cfg), C.byref(st), C.byref(prev), scratch, plan[-1].parity, _s()), "hgym_rollout_end")
    side.verify("hgym_rollout_end")
    assert int(step) == T and int(buf.counters[L.CNT_STEP]) == 397 + T
    assert sum(int(d.sum()) for d in c["dones"]) > 0, "the planted time-outs did not happen"
    if deferred:        # nobody has written these yet: the critic runs once over the stored rows, slot by slot here
        assert all(_all_ff(t) for t in c["values"] + c["priv_bf16"])
        for i in range(T):
            sh = net.shadow_struct(None, c["priv_bf16"][i])
            L.check(L.lib.hgym_critic_values(C.byref(net.cfg), C.byref(net.struct), N, L.fptr(c["priv"][i]), L.fptr(c["values"][i]), C.byref(sh),
                                             _s()), "hgym_critic_values")
            side.verify("hgym_critic_values slot %d" % i)
    else:
        assert all(_all_ff(t) for t in c["time_outs"])
        c.pop("time_outs")
    for k, v in c.items():
        for i, t in enumerate(v):
            out["%s[%d]" % (k, i)] = t
    _env_state(buf, out, "rollout.")
    if buf._l0_partial is not None and any(p.l0_ahead is not None for p in plan):
        out["l0_partial"] = buf._l0_partial
    # the evaluation launch: mu of slot T's rows, the env step on it, observations into two fresh rows
    eo, ep, act = A_.carve((N, no), F32), A_.carve((N, npv), F32), A_.carve((N, A), F32)
    L.check(L.lib.hgym_rollout_begin(C.byref(st), L.i64ptr(step), scratch, 0, _s()), "hgym_rollout_begin")
    o = buf.out_struct(eo, ep, None, True, alt=False)
    o.log_cur, o.log_stats = None, None
    watch("hgym_rollout_eval_step", 0, lambda: L.check(L.lib.hgym_rollout_eval_step(
        C.byref(net.cfg), C.byref(net.struct), C.byref(cfg), C.byref(sim), C.byref(st), C.byref(o), None, L.fptr(c["obs"][T]), L.fptr(act),
        scratch, 0, _s()), "hgym_rollout_eval_step"))
    side.verify("hgym_rollout_eval_step")
    L.check(L.lib.hgym_rollout_end(C.byref(cfg), C.byref(st), C.byref(o), scratch, 0, _s()), "hgym_rollout_end")
    side.verify("hgym_rollout_end after the evaluation launch")
    out.update(eval_obs=eo, eval_priv=ep, eval_actions=act)
    _env_state(buf, out, "eval.")
    return out


def rollout_arena_bytes(N, T, opts):
    """arena_bytes of what _rollout_sequence carves from the side's allocator (the env's own buffers have an arena of their own)."""
    no, npv, A = _dims(opts)
    ld = [_nets(opts)[0].shadow_ld(k) for k in (0, 1)]
    per_slot = [4 * N * no, 4 * N * npv]
    per_step = [2 * N * ld[0], 2 * N * ld[1]] + [4 * N * A] * 3 + [4 * N] * 3 + [N] * 2
    return G.arena_bytes(*(per_slot * (T + 1) + per_step * T + [8] + [4 * N * no, 4 * N * npv, 4 * N * A] + [4 * N * A]))


@pytest.mark.parametrize("deferred", [False, True], ids=["inline", "deferred"])
def test_fused_rollout_launches(deferred):
    """Three steps of hgym_rollout_begin / _step / _end -- with the critic's tiles inline, and in the values = NULL form followed by
    hgym_critic_values over every slot -- and one hgym_rollout_eval_step at N = 64 (the launch takes whole 32-env tiles only: at the sizes
    of the other env cases the runner's rollout_fused_mode is None).  _rollout_sequence says what is carved how.  At N = 64 every launch
    takes the 32-row layout (rollout_critic64 in csrc/hgym_rollout.hip asks for at least four tiles):
    rollout_step_kernel<0,0>, <1,1,1> twice (inline); <0,0,0,1>, <1,0,0,1> twice (deferred); <1,0,0,1,0,1> (evaluation)."""
    N, T = 64, 3
    opts = _opts("bf16-fused")
    case = _case(opts)
    _pair(lambda side: _rollout_sequence(side, N, T, deferred, opts, case), "fused rollout N=%d %s" % (N, "deferred" if deferred else "inline"),
          nbytes=96 << 20, nets=_nets(opts))


# (N, HGYM_L0_KB0): the forms of the production launch (csrc/hgym_rollout.hip).  T = 4: launches 1, 2, 3 are the steady-state launch
# (l0_ready set), with both l0 parities, launches 1 and 2 with rows ahead and launch 3 without.
#   96   3 tiles, an odd count: the 32-row layout, whose critic tiles carry the side jobs; rollout_step_kernel<1,1,1> on a (3, 3) grid
#   128  the smallest N with the 64-row layout (4 tiles): rollout_step_kernel<1,1,1,0,1>
#   320  10 grid columns: columns 8 and 9 are the first whose critic / side-job roles are swapped ((x ^ (x >> 3)) & 1)
#   128 with HGYM_L0_KB0=4: the smallest carried-first-layer split; the side jobs' staging buffer is sized by it
ROLLOUT_FORMS = [(96, None), (128, None), (320, None), (128, "4")]
WARM = 15      # env steps ahead of these rollouts: a full frame stack, so that the sums carried ahead are not sums of zeros
ROLLOUT_FORM_IDS = ["N%d%s" % (n, "-kb0_%s" % k if k else "") for n, k in ROLLOUT_FORMS]


def _assert_form(N, info, c64):
    plan, buf = info["plan"], info["buf"]
    ready = [p for p in plan if p.l0_ready is not None]
    assert len(ready) >= 2 and {p.l0_ready for p in ready} == {0, 1}, "the steady-state launch did not run with both l0 parities"
    assert any(p.ahead is not None for p in ready) and any(p.ahead is None for p in ready)
    tiles = N // 32
    assert N % 32 == 0 and ((tiles % 2 == 0 and tiles >= 4) == c64), (N, c64)
    for k in (0, 1):
        assert bool((buf.l0_partial(k) != 0).any()), "l0_partial(%d) was never written: the carried first layer did not run" % k


def _set_rollout_env(monkeypatch, kb0, critic64=None):
    for name, v in (("HGYM_L0_KB0", kb0), ("HGYM_RO_CRITIC64", critic64)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


_ROLLOUT_GUARDED = {}


@pytest.mark.parametrize("N,kb0", ROLLOUT_FORMS, ids=ROLLOUT_FORM_IDS)
def test_fused_rollout_forms(monkeypatch, N, kb0):
    """The inline rollout of test_fused_rollout_launches, T = 4, at the env counts at which the launch changes form (ROLLOUT_FORMS)."""
    T = 4
    _set_rollout_env(monkeypatch, kb0)
    opts = _opts("bf16-fused")
    case = _case(opts)
    infos = []

    def run(side):
        infos.append({})
        out = _rollout_sequence(side, N, T, False, opts, case, info=infos[-1], warm=WARM)
        _assert_form(N, infos[-1], c64=N in (128, 320))
        _ROLLOUT_GUARDED[(N, kb0)] = {k: v.clone() for k, v in out.items()}
        return out
    _pair(run, "fused rollout N=%d T=%d inline, HGYM_L0_KB0=%s" % (N, T, kb0), nbytes=rollout_arena_bytes(N, T, opts),
          nets=_nets(opts, max_batch=max(N, MAX_BATCH)))


@pytest.mark.parametrize("N", [128, 320])
def test_fused_rollout_32_row_layout_between_bands(monkeypatch, N):
    """HGYM_RO_CRITIC64=0 at the env counts where the 64-row layout is the default: the 32-row layout (rollout_step_kernel<1,1,1> on 4 and
    10 columns) stays inside the bands too, and every output has the bits of the DEFAULT layout's guarded run -- but for the carried partial
    sums themselves (12 of the 24 k-steps instead of 20) and the fp32-atomic means, as tests/test_rollout_layout_gpu.py excludes them."""
    T = 4
    opts = _opts("bf16-fused")
    case = _case(opts)
    nets = _nets(opts, max_batch=max(N, MAX_BATCH))
    if (N, None) not in _ROLLOUT_GUARDED:      # (run alone: the default layout's guarded run first)
        _set_rollout_env(monkeypatch, None)
        arena = G.Arena(DEV, rollout_arena_bytes(N, T, opts))
        side = Side("default layout N=%d" % N, arena, nets[1], (arena, nets[2]))
        _ROLLOUT_GUARDED[(N, None)] = {k: v.clone() for k, v in _rollout_sequence(side, N, T, False, opts, case, warm=WARM).items()}
        side.verify("end of the case")
    _set_rollout_env(monkeypatch, None, "0")
    info = {}
    arena = G.Arena(DEV, rollout_arena_bytes(N, T, opts))
    side = Side("fused rollout N=%d, 32-row layout" % N, arena, nets[1], (arena, nets[2]))
    got = _rollout_sequence(side, N, T, False, opts, case, info=info, warm=WARM)
    side.verify("end of the case")
    assert sum(p.l0_ready is not None for p in info["plan"]) >= 2 and bool((info["buf"].l0_partial(0) != 0).any())
    ref = dict(_ROLLOUT_GUARDED[(N, None)])
    ref.pop("l0_partial"), got.pop("l0_partial")
    _compare(ref, got, side.what)


def test_fused_rollout_any_activation():
    """A Tanh net (fused_activation): rollout_step_act_kernel (csrc/hgym_rollout_act.hip) in its three modes -- <0> first launch, <1> with the
    previous finaliser, <1, EVAL> -- at N = 64, T = 3, values deferred, then hgym_critic_values per slot (mlp_fwd_act_kernel).  The any-activation
    fused step exists without critic tiles only, so there is no inline case."""
    N, T = 64, 3
    opts = _opts("bf16-fused", act=U.TANH)
    case = _case(opts)
    _pair(lambda side: _rollout_sequence(side, N, T, True, opts, case), "fused rollout N=%d deferred, Tanh" % N,
          nbytes=rollout_arena_bytes(N, T, opts), nets=_nets(opts))
