"""-m gpu: left-right symmetry augmentation on the device -- hgym_mirror_rows bit for bit against a host expression at every layout it
takes, RolloutStorage.mirror(), the doubled update against a twin net fed columns doubled with torch, the permutation over 2 T N
rows, captured against eager updates, and the feature switched off."""
import copy
import ctypes as C

import pytest
import torch

from update_options_common import _alg, _fill_rollout, _record_batches      # the update harness, shared with tests/test_update_options_gpu.py

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = (1, 12, 47, 219, 705)
ROWS = (1, 63, 64, 65, 257, 1000)
GUARD = 64


def _int_dtype(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


def _sign_mask(sign, dtype):
    """The element's sign bit where sign < 0, as the signed integer of the element's width."""
    top = -(1 << 31) if dtype == torch.float32 else -(1 << 15)
    return torch.where(sign < 0, torch.full_like(sign, top, dtype=torch.int64), torch.zeros_like(sign, dtype=torch.int64)).to(_int_dtype(dtype))


def _mirror_bits(x, src_col, sign):
    """The host expression: x (M, width) float32 / bfloat16 -> same dtype, x.view(int)[:, src_col] ^ signmask."""
    return (x.contiguous().view(_int_dtype(x.dtype))[:, src_col.long()] ^ _sign_mask(sign, x.dtype)).view(x.dtype)


def _random_bits(g, n, dtype):
    """n elements of uniformly random bit patterns (NaNs with payloads, infinities, denormals among them by construction of the
    format: ~0.4 % of fp32 patterns have an all-ones exponent, ~0.4 % an all-zero one), the special values planted up front."""
    it = _int_dtype(dtype)
    lo, hi = (-(1 << 31), 1 << 31) if it == torch.int32 else (-(1 << 15), 1 << 15)
    bits = torch.randint(lo, hi, (n,), dtype=torch.int64, device=DEV, generator=g).to(it)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan"), 1e-40, -1e-40, 1.0, -2.5],
                           dtype=torch.float32, device=DEV).to(dtype).view(it)
    k = min(n, special.numel())
    bits[:k] = special[:k]
    if n > 40:       # ... and once more further in, so that wide rows carry them in other columns too
        bits[30:40] = special
    return bits


def _tables(g, width):
    from humanoid.utils.symmetry import xbot_l_frames, xbot_l_mirror
    from types import SimpleNamespace
    ident = (torch.arange(width), torch.ones(width))
    rnd = (torch.randperm(width, generator=torch.Generator().manual_seed(width)), torch.randint(0, 2, (width,), generator=torch.Generator().manual_seed(width + 1)) * 2.0 - 1.0)
    spec = xbot_l_mirror(SimpleNamespace(env=SimpleNamespace(frame_stack=15, c_frame_stack=3, num_single_obs=47, single_num_privileged_obs=73, num_actions=12),
                                         terrain=SimpleNamespace(measure_heights=False)))
    xbot = {12: (spec.act_src, spec.act_sign), 47: xbot_l_frames()[0], 219: (spec.priv_src, spec.priv_sign), 705: (spec.obs_src, spec.obs_sign),
            1: ([0], [-1])}[width]
    out = {}
    for name, (s, sg) in (("identity", ident), ("xbot_l", xbot), ("random", rnd)):
        out[name] = (torch.as_tensor(s).to(torch.int32).to(DEV), torch.as_tensor(sg).to(torch.float32).to(DEV))
    return out


def _layout(kind, width):
    """-> (ld_src, ld_dst, zero_to, rows the source view is offset by)."""
    if kind == "contiguous":          # odd row sizes, the source one row into its buffer: rows start only 4- / 2-byte aligned
        return width, width, width, 1
    if kind == "ragged":              # ld_src != ld_dst, two pad columns zeroed, three columns of every dst row not touched
        return width + 3, width + 5, width + 2, 1
    ld = (width + 127) // 128 * 128   # "shadow": 16-byte aligned rows, every pad column zeroed
    return ld, ld, ld, 0


@pytest.mark.parametrize("kind", ["contiguous", "ragged", "shadow"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mirror_rows_equals_the_host_expression_bit_for_bit(dtype, kind):
    import hgym
    it = _int_dtype(dtype)
    fill = 0x7FFF7FFF if dtype == torch.float32 else 0x7FFF
    g = torch.Generator(device=DEV).manual_seed(11)
    for width in WIDTHS:
        tables = _tables(g, width)
        ld_src, ld_dst, zero_to, off = _layout(kind, width)
        for M in ROWS:
            sbuf = _random_bits(g, (M + off) * ld_src, dtype).view(M + off, ld_src)
            src = sbuf[off:].view(dtype)[:, :width] if ld_src > width else sbuf[off:].view(dtype)
            front = GUARD + (1 if kind != "shadow" else 0)       # (one more element: the destination rows start element-aligned only)
            for name, (src_col, sign) in tables.items():
                dbuf = torch.full((front + M * ld_dst + GUARD,), fill, dtype=it, device=DEV)
                want = dbuf.clone()
                w = want[front:front + M * ld_dst].view(M, ld_dst)
                w[:, :width] = sbuf[off:, :width][:, src_col.long()] ^ _sign_mask(sign, dtype)
                w[:, width:zero_to] = 0
                dst = dbuf[front:front + M * ld_dst].view(M, ld_dst).view(dtype)
                hgym.mirror_rows(src, dst if ld_dst == width else dst[:, :width], src_col, sign, zero_to=zero_to)
                assert torch.equal(dbuf, want), (dtype, kind, width, M, name, int((dbuf != want).sum()))
                if name == "identity":
                    assert torch.equal(dbuf[front:front + M * ld_dst].view(M, ld_dst)[:, :width], sbuf[off:, :width])
    torch.cuda.synchronize()


def test_mirror_rows_refuses_bad_arguments_without_launching():
    from hgym import _lib as L
    M, W, LD = 8, 12, 16
    src = torch.randn(M, LD, device=DEV)
    dst = torch.full((M, LD), 7.0, device=DEV)
    col = torch.arange(W, dtype=torch.int32, device=DEV)
    sign = -torch.ones(W, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    ip = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int32))
    ok = dict(M=M, width=W, col=ip(col), sign=L.fptr(sign), src=p(src), ld_src=LD, dst=p(dst), ld_dst=LD, zero_to=W, dtype=L.F32)

    def call(**over):
        a = dict(ok, **over)
        return L.lib.hgym_mirror_rows(a["M"], a["width"], a["col"], a["sign"], a["src"], a["ld_src"], a["dst"], a["ld_dst"], a["zero_to"], a["dtype"],
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [dict(col=None), dict(sign=None), dict(src=None), dict(dst=None), dict(width=0), dict(width=-3), dict(ld_src=W - 1), dict(ld_dst=W - 1),
           dict(zero_to=W - 1), dict(zero_to=LD + 1), dict(dtype=2), dict(dtype=-1), dict(M=-1),
           dict(dst=C.c_void_p(src.data_ptr() + 4 * LD)),                       # dst starts inside src
           dict(dst=C.c_void_p(src.data_ptr() - 4 * LD * (M - 1) - 4 * W + 4)),  # dst ends inside src (its last written element is src[0][0])
           dict(src=C.c_void_p(src.data_ptr() + 2))]                            # not aligned to the element
    for over in bad:
        assert call(**over) == -1, over       # HGYM_E_BADARG
        assert L.lib.hgym_last_error()
    assert call(width=L.MIRROR_MAX_WIDTH + 1, ld_src=4096, ld_dst=4096, zero_to=L.MIRROR_MAX_WIDTH + 1) == -4       # HGYM_E_UNSUPPORTED
    assert call(M=0) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    assert call() == 0                        # ... and the same arguments unmodified do run
    torch.cuda.synchronize()
    assert torch.equal(dst[:, :W], -src[:, :W]) and bool((dst[:, W:] == 7.0).all())


# ---------------------------------------------------------------------------------------------- storage
def _spec():
    from humanoid.envs import task_registry      # noqa: F401
    from humanoid.utils import task_registry as reg
    from humanoid.utils.symmetry import xbot_l_mirror
    return xbot_l_mirror(reg.get_cfgs("humanoid_ppo")[0])


def _dev_tables(spec):
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    return dict(obs=(t(spec.obs_src, torch.int32), t(spec.obs_sign, torch.float32)), priv=(t(spec.priv_src, torch.int32), t(spec.priv_sign, torch.float32)),
                act=(t(spec.act_src, torch.int32), t(spec.act_sign, torch.float32)), sigma=(t(spec.act_src, torch.int32), torch.ones(12, device=DEV)))


def test_storage_mirror_fills_the_second_half_and_nothing_else():
    from humanoid.algo.ppo.rollout_storage import RolloutStorage
    T, N = 3, 64
    spec = _spec()
    st = RolloutStorage(N, T, [705], [219], [12], DEV)
    plain = {k: tuple(v.shape) for k, v in vars(st).items() if torch.is_tensor(v)}
    assert st.enable_mirror(spec) and st.enable_shadow(768, 256) and st.mirrored
    assert {k: tuple(v.shape) for k, v in vars(st).items() if torch.is_tensor(v) and k in plain} == plain      # the public views keep their shapes
    g = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda t: t.copy_(torch.randn(t.shape, device=DEV, generator=g))
    stores = dict(obs=st._obs_store, priv=st._priv_store, **st._col_store)
    for t in stores.values():
        rnd(t)                                                   # every slot, the mirrored half included: distinct random values
    for sh, full in ((st._obs_bf16_store, st._obs_store), (st._priv_bf16_store, st._priv_store)):
        sh.fill_(3.0)                                            # (pads of the mirrored half: must come out +0)
        sh[:T].zero_()
        sh[:T, :, :full.shape[2]] = full[:T].to(torch.bfloat16)  # what the policy launches leave
    st.shadow_valid = [True] * T
    before = {k: v.clone() for k, v in stores.items()}
    sh_before = (st._obs_bf16_store.clone(), st._priv_bf16_store.clone())
    st.mirror()
    torch.cuda.synchronize()
    tab = _dev_tables(spec)
    fl = lambda t: t.flatten(0, 1)
    bits = lambda t: t.contiguous().view(_int_dtype(t.dtype))
    for name, table in (("obs", "obs"), ("priv", "priv"), ("actions", "act"), ("mu", "act"), ("sigma", "sigma")):
        want = _mirror_bits(fl(before[name][:T]), *tab[table])
        assert torch.equal(bits(fl(stores[name][T + 1:])), bits(want)), name
    for name in ("values", "returns", "advantages", "actions_log_prob"):
        assert torch.equal(bits(stores[name][T + 1:]), bits(before[name][:T])), name
    for name in stores:                                          # the rollout itself and slot T: only read
        assert torch.equal(bits(stores[name][:T + 1]), bits(before[name][:T + 1])), name
    for sh, was, full, w in ((st._obs_bf16_store, sh_before[0], st._obs_store, 705), (st._priv_bf16_store, sh_before[1], st._priv_store, 219)):
        assert torch.equal(bits(sh[:T + 1]), bits(was[:T + 1]))
        assert torch.equal(bits(sh[T + 1:, :, :w]), bits(full[T + 1:].to(torch.bfloat16)))       # = bfloat16(mirrored fp32 rows)
        assert bool((bits(sh[T + 1:, :, w:]) == 0).all())
    # the public views are the first T slots of the same memory
    assert st.observations.data_ptr() == st._obs_store.data_ptr() and st.actions.data_ptr() == st._col_store["actions"].data_ptr()
    assert st._obs_all.shape == (T + 1, N, 705) and st._obs_bf16.shape == (T, N, 768)


# ---------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_first_minibatch_gradient_equals_a_twin_on_columns_doubled_with_torch(monkeypatch, precision):
    import hgym
    T, N = 4, 64
    spec = _spec()
    alg = _alg(monkeypatch, precision, N, T, spec)
    st = alg.storage
    assert st.mirrored and alg.net.cfg.max_batch == 2 * T * N // 2
    _fill_rollout(alg, 31)
    assert (st.shadows() is not None) == (precision == "bf16")
    p0 = alg.net.params.clone()
    fl = lambda t: t.flatten(0, 1).clone()
    cols0 = dict(obs=fl(st.observations), priv=fl(st.privileged_observations), actions=fl(st.actions), mu=fl(st.mu), sigma=fl(st.sigma),
                 values=fl(st.values), returns=fl(st.returns), advantages=fl(st.advantages), actions_log_prob=fl(st.actions_log_prob))
    idx_log, grad_log = _record_batches(monkeypatch, alg)
    alg.update()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(idx_log) == 2 and idx_log[0].numel() == T * N
    idx = idx_log[0]
    assert bool(((idx < T * N) | ((idx >= (T + 1) * N) & (idx < (2 * T + 1) * N))).all())
    rows = torch.where(idx >= (T + 1) * N, idx - N, idx).contiguous()      # plain row numbers of [0, 2 T N)
    assert int((rows >= T * N).sum()) > 0 and int((rows < T * N).sum()) > 0

    # the twin: no symmetry, 2 T slots holding [rollout | rollout mirrored with torch], the same parameters
    twin = _alg(monkeypatch, precision, N, 2 * T, None)
    assert not twin.storage.mirrored and twin.net.cfg.max_batch == alg.net.cfg.max_batch
    twin.net.params.copy_(p0)
    twin.net.sync_shadow()
    tab = _dev_tables(spec)
    table_of = dict(obs="obs", priv="priv", actions="act", mu="act", sigma="sigma")      # (the scalar columns are repeated unchanged)
    doubled = {k: torch.cat((v, _mirror_bits(v, *tab[table_of[k]]) if k in table_of else v)) for k, v in cols0.items()}
    s2 = twin.storage
    for name, attr in (("obs", "observations"), ("priv", "privileged_observations")) + tuple((k, k) for k in s2.MIRRORED):
        getattr(s2, attr).flatten(0, 1).copy_(doubled[name])
    sh = {}
    if precision == "bf16":
        for full, shadow in ((doubled["obs"], s2._obs_bf16), (doubled["priv"], s2._priv_bf16)):
            shadow.zero_()
            shadow.flatten(0, 1)[:, :full.shape[1]] = full.to(torch.bfloat16)
        s2.shadow_valid = [True] * (2 * T)
        sh = dict(zip(("obs_bf16", "priv_bf16"), s2.shadows()))
    twin.net.ppo_grad(twin._ppo_cfg, hgym.make_batch(*s2.batch_columns(), rows, **sh))
    torch.cuda.synchronize()
    assert float(grad_log[0].abs().max()) > 0
    assert torch.equal(twin.net.grads.view(torch.int32), grad_log[0].view(torch.int32))


def test_permutation_covers_both_halves_once_per_epoch_and_never_slot_T(monkeypatch):
    T, N = 4, 64
    alg = _alg(monkeypatch, "f32", N, T, _spec(), epochs=2)
    idx_log, _ = _record_batches(monkeypatch, alg)
    valid = torch.cat((torch.arange(T * N), torch.arange((T + 1) * N, (2 * T + 1) * N))).to(DEV)
    draws = []
    for it in range(2):
        _fill_rollout(alg, 40 + it)
        alg.update()
        got = idx_log[4 * it:4 * it + 4]
        assert len(got) == 4 and all(i.numel() == T * N for i in got)
        for epoch in range(2):
            rows = torch.cat(got[2 * epoch:2 * epoch + 2])
            assert torch.equal(torch.sort(rows)[0], valid), (it, epoch)       # each of the 2 T N rows once, none in slot T
        draws.append(torch.cat(got[:2]))
    assert not torch.equal(draws[0], draws[1])       # a new draw per update


# ---------------------------------------------------------------------------------------------- runner
TASK = "humanoid_ppo"


def _runner(num_envs, seed, symmetry, steps=8):
    from humanoid.algo import PPO
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    PPO.precision = "bf16"
    args = get_args(["--task=" + TASK, "--headless", "--num_envs", str(num_envs), "--seed", str(seed)])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=TASK))
    env_cfg.seed = train_cfg.seed = seed
    train_cfg.runner.num_steps_per_env = steps
    if symmetry is not None:
        train_cfg.algorithm.symmetry = symmetry
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=copy.deepcopy(env_cfg))
    runner, _ = task_registry.make_alg_runner(env=env, args=args, train_cfg=train_cfg, log_root=None)
    return runner


def test_captured_update_with_symmetry_equals_the_eager_one(monkeypatch):
    out = {}
    for graph_update in ("1", "0"):
        monkeypatch.setenv("HGYM_GRAPH_UPDATE", graph_update)
        torch.manual_seed(97)
        r = _runner(64, 23, True)
        assert r.alg.storage.mirrored and r.alg._symmetry is not None
        r.learn(num_learning_iterations=3, init_at_random_ep_len=False)
        torch.cuda.synchronize()
        assert (r._update_graph is not None) == (graph_update == "1")
        out[graph_update] = (r.alg.net.params.clone(), r.alg.net.opt_state.clone(), r.alg.net.adam_m.clone())
        del r
    for a, b in zip(out["1"], out["0"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    from hgym import _lib as L
    assert float(out["1"][1][L.OPT_STEP]) == 3 * 2 * 4      # iterations x epochs x minibatches: as many Adam steps as without the feature


@pytest.mark.parametrize("symmetry", [None, False])
def test_switched_off_nothing_changes(monkeypatch, symmetry):
    from hgym import _lib as L
    calls = []
    real = L.lib.hgym_mirror_rows

    def counting(*a):
        calls.append(a)
        return real(*a)
    monkeypatch.setattr(L.lib, "hgym_mirror_rows", counting)
    torch.manual_seed(98)
    r = _runner(64, 24, symmetry)
    st, T, N = r.alg.storage, 8, 64
    r.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    torch.cuda.synchronize()
    assert calls == [] and not st.mirrored and r.alg._symmetry is None
    shapes = dict(_obs_all=(T + 1, N, 705), _priv_all=(T + 1, N, 219), observations=(T, N, 705), privileged_observations=(T, N, 219),
                  rewards=(T, N, 1), actions=(T, N, 12), dones=(T, N, 1), actions_log_prob=(T, N, 1), values=(T, N, 1), returns=(T, N, 1),
                  advantages=(T, N, 1), mu=(T, N, 12), sigma=(T, N, 12), _obs_bf16=(T, N, 768), _priv_bf16=(T, N, 256))
    for name, shape in shapes.items():
        t = getattr(st, name)
        assert tuple(t.shape) == shape, name
        base = getattr(st, "_obs_all" if name == "observations" else "_priv_all" if name == "privileged_observations" else name)
        assert t.untyped_storage().nbytes() == base.numel() * base.element_size(), name       # no room for a second half either
    assert r.alg.net.cfg.max_batch == T * N // 4
