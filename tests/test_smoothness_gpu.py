"""-m gpu: the smoothness regulariser at the library level (hgym_smooth_pairs, hgym_perturb_rows, hgym_ppo_grad_smooth; DESIGN.md section
28) against tests/smoothness_common.py's float64 reference and numpy restatements.

1. hgym_perturb_rows: the Philox block of slot 128 against oracle/philox.py at tests/test_philox.py's device bar, src + noise_std * z to one
   fp32 rounding, zero-noise columns and repeated calls bit for bit, the padding columns +0.0, other bits after one more Adam step.
2. hgym_smooth_pairs against the numpy restatement, bit for bit.
3. The gradient and the sums of every instantiation (all three paths, fp32 rows and the bf16 shadow, ELU(1) and Tanh, both value-loss
   forms, each term alone and both) at the project's bars; everything but the actor's gradient torch.equal hgym_ppo_grad's on the same
   inputs.  The reference is fed the perturbed rows the device wrote.
4. Off is off: both coefficients 0, and lamS = 0 with every row done, give hgym_ppo_grad's bits.
5. Batch edges B in {1, 63, 64, 65} on the fused path.
6. Misuse is refused with HGYM_E_BADARG and nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

import smoothness_common as S
import update_options_common as U
import test_update_options_gpu as G
from hgym import _lib as L

pytestmark = pytest.mark.gpu

O = U.Options
FUSED = [O("bf16-fused", act, "scalar", vu, False, False, sh) for act in (None, U.TANH) for vu in (False, True) for sh in (False, True)]
LAYER = [O(p, act, "scalar", False, False, False, False) for p in ("f32-layer", "bf16-layer") for act in (None, U.TANH)]
EXTRA = [O("bf16-fused", None, "log", False, False, False, True), O("bf16-fused", None, "scalar", False, True, False, True),
         O("bf16-fused", U.TANH, "log", True, True, True, False), O("f32-layer", None, "scalar", True, False, True, False)]
CASES = FUSED + LAYER + EXTRA
ALONE = [O(p, None, "scalar", False, False, False, p == "bf16-fused") for p in U.PATHS]
STEP = 3      # opt_state[HGYM_OPT_STEP] of every gradient case: the Philox step word
PHILOX_ATOL = 2e-5      # tests/test_philox.py's device bar


def _opt(step):
    o = torch.zeros(L.OPT_STATE, dtype=torch.float64, device="cuda")
    o[L.OPT_STEP] = float(step)
    return o


# ---------------------------------------------------------------------------------------------- 1. hgym_perturb_rows
@pytest.mark.parametrize("gathered", [False, True], ids=["contiguous", "gathered"])
@pytest.mark.parametrize("M", [1, 63, 130])
@pytest.mark.parametrize("width", [5, 47, 705])
def test_perturb_rows(width, M, gathered):
    import hgym
    g = torch.Generator().manual_seed(1000 * width + M)
    rows_stored = 3 * M + 7
    idx_h = torch.randperm(rows_stored, generator=g)[:M].contiguous() if gathered else None
    row_of = idx_h.numpy() if gathered else np.arange(M)
    idx = idx_h.cuda() if gathered else None
    ld_src, ld = width + 3, hgym.smooth_ld(width)
    ns_h = (0.1 + torch.rand(width, generator=g)).float()
    ns_h[::4] = 0.0
    ns = ns_h.cuda()
    ones = torch.ones(width, device="cuda")
    step, seed = 11, S.SEED
    src0 = torch.full((rows_stored, ld_src), float("nan"), device="cuda")      # the tail of every row is never read
    src0[:, :width] = 0.0

    def run(src, noise, opt):
        dst = torch.full((M + 2, ld), float("nan"), device="cuda")
        hgym.perturb_rows(src[:, :width], noise, seed, opt, dst[:M], idx=idx)
        torch.cuda.synchronize()
        assert torch.isnan(dst[M:]).all()      # rows behind M untouched
        return dst[:M]
    # src = 0, noise_std = 1: the normals themselves
    z_dev = run(src0, ones, _opt(step))[:, :width].cpu().numpy()
    z_ref = S.normals(seed, step, row_of, width)
    print("perturb width=%d M=%d: max |z_dev - z_oracle| = %.3e (bar %.1e)" % (width, M, np.abs(z_dev - z_ref).max(), PHILOX_ATOL))
    np.testing.assert_allclose(z_dev, z_ref, rtol=0, atol=PHILOX_ATOL)
    # random src: src + noise_std * z_dev to one fp32 rounding, zero-noise columns bit for bit, the padding +0.0
    src = src0.clone()
    x_h = torch.randn(rows_stored, width, generator=g)
    x_h[0, 0] = -0.0
    src[:, :width] = x_h.cuda()
    out = run(src, ns, _opt(step))
    got = out[:, :width].cpu().numpy()
    xs = x_h.numpy()[row_of]
    exact = xs.astype(np.float64) + ns_h.numpy().astype(np.float64)[None, :] * z_dev.astype(np.float64)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    on = ns_h.numpy() != 0
    assert (np.abs(got.astype(np.float64) - exact)[:, on] <= ulp[:, on]).all()
    assert np.array_equal(got[:, ~on].view(np.uint32), xs[:, ~on].view(np.uint32))
    assert bool((out[:, width:].contiguous().view(torch.int32) == 0).all())
    assert np.isfinite(got).all()
    # the same bits from a second call; other bits one Adam step later and under another seed word
    again = run(src, ns, _opt(step))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    later = run(src, ns, _opt(step + 1))[:, :width].cpu().numpy()
    assert not np.array_equal(later[:, on], got[:, on]), "the step word is ignored"
    assert np.array_equal(later[:, ~on].view(np.uint32), got[:, ~on].view(np.uint32))
    z_later = run(src0, ones, _opt(step + 1))[:, :width].cpu().numpy()
    np.testing.assert_allclose(z_later, S.normals(seed, step + 1, row_of, width), rtol=0, atol=PHILOX_ATOL)


# ---------------------------------------------------------------------------------------------- 2. hgym_smooth_pairs
@pytest.mark.parametrize("T,N,B", [(4, 3, 1), (6, 5, 30), (60, 64, 3840), (9, 33, 257)])
def test_smooth_pairs(T, N, B):
    import hgym
    g = torch.Generator().manual_seed(T * N + B)
    dones = (torch.rand(T * N, generator=g) < 0.4).to(torch.uint8)
    idx = torch.randperm(T * N, generator=g)[:B].contiguous()
    nxt = torch.full((B + 3,), -7, dtype=torch.int64, device="cuda")
    w = torch.full((B + 3,), float("nan"), device="cuda")
    hgym.smooth_pairs(idx.cuda(), dones.cuda(), N, nxt[:B], w[:B])
    torch.cuda.synchronize()
    rn, rw = S.successor(idx.numpy(), dones.numpy(), N)
    assert np.array_equal(nxt[:B].cpu().numpy(), rn) and np.array_equal(w[:B].cpu().numpy().view(np.uint32), rw.view(np.uint32))
    assert bool((nxt[B:] == -7).all()) and torch.isnan(w[B:]).all()


# ---------------------------------------------------------------------------------------------- 3. the gradient
def _grad(net, opts, case, ppo, shadow, lam=(S.LAM_T, S.LAM_S), rows=128, plain=False, weight=None):
    """One hgym_ppo_grad_smooth (plain: hgym_ppo_grad) + the unfold on the case.  -> (sums, target_next, target_near, perturbed rows), the
    scratch NaN behind the minibatch's rows.  The successor map comes from hgym_smooth_pairs on the case's dones."""
    import hgym
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    no, A, B = cols[0].shape[1], cols[2].shape[1], case["B"]
    ld = hgym.smooth_ld(no)
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    tn, ts, pr = nan(rows * A), nan(rows * A), nan(rows * ld)
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    idx = case["idx"].cuda()
    nxt, w = torch.empty(B, dtype=torch.int64, device="cuda"), torch.empty(B, device="cuda")
    hgym.smooth_pairs(idx, torch.from_numpy(case["dones"]).cuda(), case["N"], nxt, w)
    if weight is not None:
        w.copy_(weight)
    net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
    net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
    net.opt_state[L.OPT_STEP] = float(STEP)
    batch = hgym.make_batch(*cols, idx, **kw)
    if plain:
        net.ppo_grad(ppo, batch)
    else:
        sm = hgym.make_smooth(lam[0], lam[1], next_idx=nxt, next_weight=w, noise_std=torch.from_numpy(case["noise_std"]).cuda(), seed=S.SEED,
                              target_next=tn, target_near=ts, rows=pr, sums=sums)
        net.ppo_grad_smooth(ppo, batch, sm)
    if opts.norm:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    assert np.array_equal(nxt.cpu().numpy(), case["nxt"].numpy())
    return sums.cpu(), tn, ts, pr.view(rows, ld)


def _hold(what, opts, errs, bar):
    print("\n%s" % what)
    for k, e in errs.items():
        print("    %-20s %.3e  (bar %.1e)%s" % (k, e, bar, "  <-- above" if not e <= bar else ""))
    worst = max(errs, key=lambda k: errs[k] if errs[k] == errs[k] else float("inf"))
    assert errs[worst] <= bar, "%s: %s measured %.3e > bar %.1e" % (what, worst, errs[worst], bar)


OPT_KEPT = (L.OPT_LR, L.OPT_STEP, L.OPT_KL_SUM, L.OPT_SURROGATE_SUM, L.OPT_VALUE_SUM, L.OPT_ENTROPY_SUM, L.OPT_MINIBATCHES, L.OPT_KL_LAST,
            L.OPT_AUX_SUM)


def _others_keep_their_bits(net, g0, o0, expect_actor_moved=True):
    """Everything but the actor's gradient -- d std, the critic, the auxiliary head, the KL slot, the loss sums -- against the plain run."""
    views, base = net.views, net.params.data_ptr()
    flat0, flat1 = g0[:net.P], net.grads_ext[:net.P]
    moved = 0
    for k, v in views.items():
        o = (v.data_ptr() - base) // 4
        a, b = flat0[o:o + v.numel()], flat1[o:o + v.numel()]
        if k.startswith("actor."):
            moved += int(not torch.equal(a, b))
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s moved with the regulariser on" % k
    if expect_actor_moved:
        assert moved == len([k for k in views if k.startswith("actor.")])
    assert torch.equal(g0[net.P:].view(torch.int32), net.grads_ext[net.P:].view(torch.int32))      # the KL slot
    for slot in OPT_KEPT:
        assert float(o0[slot]) == float(net.opt_state[slot]), slot


def _check(opts, case, lam, shadow):
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    _grad(net, opts, case, ppo, shadow, plain=True)
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    sums, tn, ts, pr = _grad(net, opts, case, ppo, shadow, lam=lam)
    assert torch.isfinite(net.grads_ext).all()
    B, A, no = case["B"], case["cols"][2].shape[1], case["cols"][0].shape[1]
    near = None
    if lam[1] > 0:
        assert torch.isfinite(pr[:B]).all() and torch.isnan(pr[B:]).all() and bool((pr[:B, no:] == 0).all())
        assert torch.isfinite(ts[:B * A]).all() and torch.isnan(ts[B * A:]).all()
        near = pr[:B, :no].cpu()
        host = S.clean_near(case, step=STEP)      # the device's rows are the restated ones up to the normals' device bar
        assert float((near - host).abs().max()) <= PHILOX_ATOL * float(case["noise_std"].max()) * 1.01 + 1e-6
    else:
        assert torch.isnan(pr).all() and torch.isnan(ts).all()      # a term that is off writes nothing
    if lam[0] > 0:
        assert torch.isfinite(tn[:B * A]).all() and torch.isnan(tn[B * A:]).all()
    else:
        assert torch.isnan(tn).all()
    ref = S.reference(case, lam_t=lam[0], lam_s=lam[1], near=near)
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    what = "smoothness lam=%s %s" % (lam, U.case_id(opts))
    _hold("%s: gradient vs float64 reference" % what, opts, U.errors(opts, got, ref), U.bar_of(opts))
    _hold("%s: loss sums" % what, opts, U.sum_errors(opts, G._sums(net), ref), U.SUM_TOL[opts.path])
    tol = U.SUM_TOL[opts.path]
    for k, on in ((0, lam[0] > 0), (1, lam[1] > 0)):
        if on and ref["smooth"][k] == 0.0:      # (B = 1: the one row is done)
            assert float(sums[k]) == 0.0
        elif on:
            err = abs(float(sums[k]) - ref["smooth"][k]) / ref["smooth"][k]
            print("    sums[%d] %.6e vs %.6e: rel %.3e (bar %.1e)" % (k, float(sums[k]), ref["smooth"][k], err, tol))
            assert err <= tol
        else:
            assert float(sums[k]) == 0.0
    assert float(sums[2]) == ref["smooth"][2] and float(sums[3]) == 1.0      # (the weights are summed whichever term is on)
    _others_keep_their_bits(net, g0, o0)
    return net, ppo


@pytest.mark.parametrize("opts", CASES, ids=[U.case_id(o) for o in CASES])
def test_gradient_and_sums_of_every_instantiation(opts):
    case = S.case_of(opts)
    S.check_mask(case)
    net, ppo = _check(opts, case, (S.LAM_T, S.LAM_S), opts.shadow)
    if opts.shadow:      # the bf16 shadow rows and the fp32 rows give the same bits
        ext = net.grads_ext.clone()
        _grad(net, opts, case, ppo, False)
        assert torch.equal(ext.view(torch.int32), net.grads_ext.view(torch.int32))


@pytest.mark.parametrize("term", ["temporal", "spatial"])
@pytest.mark.parametrize("opts", ALONE + [FUSED[4]], ids=[U.case_id(o) for o in ALONE + [FUSED[4]]])
def test_each_term_alone(opts, term):
    _check(opts, S.case_of(opts), (S.LAM_T, 0.0) if term == "temporal" else (0.0, S.LAM_S), opts.shadow)


# ---------------------------------------------------------------------------------------------- 4. off is off
@pytest.mark.parametrize("opts", ALONE + [FUSED[5]], ids=[U.case_id(o) for o in ALONE + [FUSED[5]]])
def test_off_is_off(opts):
    case = S.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case)
    _grad(net, opts, case, ppo, opts.shadow, plain=True)
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    same = lambda: (torch.equal(g0.view(torch.int32), net.grads_ext.view(torch.int32)) and
                    torch.equal(o0.view(torch.int64), net.opt_state.view(torch.int64)))
    sums, tn, ts, pr = _grad(net, opts, case, ppo, opts.shadow, lam=(0.0, 0.0))
    assert same() and float(sums.abs().sum()) == 0.0 and torch.isnan(tn).all() and torch.isnan(ts).all() and torch.isnan(pr).all()
    # lamS = 0 and every row done: the temporal term weighs nothing
    sums, tn, ts, pr = _grad(net, opts, case, ppo, opts.shadow, lam=(S.LAM_T, 0.0), weight=torch.zeros(case["B"], device="cuda"))
    assert torch.equal(g0.view(torch.int32), net.grads_ext.view(torch.int32))
    for slot in OPT_KEPT + (L.OPT_GRAD_SQNORM,):
        assert float(o0[slot]) == float(net.opt_state[slot]), slot
    assert float(sums[0]) == 0.0 and float(sums[2]) == 0.0 and float(sums[3]) == 1.0


# ---------------------------------------------------------------------------------------------- 5. batch edges
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_fused_batch_edges(B):
    opts = O("bf16-fused", None, "scalar", False, False, False, True)
    case = S.make_case(opts, seed=60 + B, B=B)
    _check(opts, case, (S.LAM_T, S.LAM_S), True)


@pytest.mark.parametrize("path", ["f32-layer", "bf16-layer"])
def test_layer_batch_edges(path):
    opts = O(path, None, "scalar", True, False, False, False)      # (unclipped: one row's d V is never 0, the last critic bias's metric is defined)
    for B in (1, 31):
        _check(opts, S.make_case(opts, seed=80 + B, B=B), (S.LAM_T, S.LAM_S), False)


# ---------------------------------------------------------------------------------------------- 6. misuse
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_misuse_is_refused(opts):
    import hgym
    case = S.case_of(opts)
    net = G._net(opts)
    G._load(net, opts, case)
    cols = [t.cuda().contiguous() for t in case["cols"]]
    no, A, B = cols[0].shape[1], cols[2].shape[1], case["B"]
    ld = hgym.smooth_ld(no)
    tn, ts, pr = (torch.zeros(n + 4, device="cuda") for n in (128 * A, 128 * A, 128 * ld))
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    idx, nxt, w = case["idx"].cuda(), case["nxt"].cuda(), case["weight"].cuda()
    ns = torch.from_numpy(case["noise_std"]).cuda()
    batch = hgym.make_batch(*cols, idx)
    net.grads_ext.fill_(7.0)
    torch.cuda.synchronize()

    def good(lt=S.LAM_T, ls=S.LAM_S):
        sm = L.Smooth()
        sm.temporal_coef, sm.spatial_coef, sm.seed = lt, ls, 5
        sm.next_idx, sm.next_weight, sm.noise_std = L.i64ptr(nxt), L.fptr(w), L.fptr(ns)
        sm.target_next, sm.target_near, sm.rows, sm.sums = L.fptr(tn), L.fptr(ts), L.fptr(pr), L.f64ptr(sums)
        return sm

    def rc(sm, ppo=None, b=batch):
        ppo = ppo or G._ppo(opts, case)
        return int(L.lib.hgym_ppo_grad_smooth(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(b), C.byref(sm), net.stream()))
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert rc(good(lt=bad)) == -1 and b"temporal_coef" in L.lib.hgym_last_error()
        assert rc(good(ls=bad)) == -1 and b"spatial_coef" in L.lib.hgym_last_error()
    for field in ("next_idx", "next_weight", "noise_std", "target_next", "target_near", "rows", "sums"):
        sm = good()
        setattr(sm, field, None)
        assert rc(sm) == -1, field
    for field, t in (("target_next", tn), ("target_near", ts), ("rows", pr)):
        sm = good()
        setattr(sm, field, C.cast(t.data_ptr() + 4, L.c_float_p))      # not 16-byte aligned
        assert rc(sm) == -1 and b"16-byte" in L.lib.hgym_last_error(), field
    assert rc(good(), ppo=G._ppo(opts, case, mirror_coef=0.5)) == -1 and b"mirror_coef" in L.lib.hgym_last_error()
    two = G._ppo(opts, case)
    two.world_size = 2
    assert rc(good(), ppo=two) == -1 and b"world_size" in L.lib.hgym_last_error()
    torch.cuda.synchronize()
    assert bool((net.grads_ext == 7.0).all()) and float(sums.sum()) == 0.0      # nothing was launched
    assert float(tn.abs().sum()) == 0.0 and float(ts.abs().sum()) == 0.0 and float(pr.abs().sum()) == 0.0
    # a term that is off needs none of its pointers
    sm = good(ls=0.0)
    sm.noise_std, sm.target_near, sm.rows = None, None, None
    assert rc(sm) == 0
    sm = good(lt=0.0)
    sm.next_idx, sm.next_weight, sm.target_next = None, None, None
    assert rc(sm) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads_ext).all() and float(sums[3]) == 2.0
