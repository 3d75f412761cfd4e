"""-m gpu: hgym_ppo_grad_smooth_mirror -- the mirror loss and the smoothness regulariser in one actor head -- at the
library level, against tests/mirror_smooth_common.py's float64 reference and against the single-option calls.

1. The gradient and the three sums of every instantiation (all three paths, fp32 rows and the bf16 shadow -- the same bits --, ELU(1) and
   Tanh, log std, the unclipped value loss, the auxiliary head, norm) at U.bar_of(opts) and U.SUM_TOL.  The reference is fed the perturbed
   rows the device wrote.
2. In the same run: mirror_sums bit for bit hgym_ppo_grad's with mirror_coef alone, smooth->sums[0..3] bit for bit hgym_ppo_grad_smooth's
   at mirror_coef 0, on the same inputs and the same OPT_STEP.
3. In the same run: everything but the actor's gradient -- d std, critic, auxiliary head, KL slot, loss sums -- torch.equal plain
   hgym_ppo_grad's.
4. Degenerate forms, bitwise: mirror_coef 0 is hgym_ppo_grad_smooth; both smoothness coefficients 0 is hgym_ppo_grad with the mirror loss;
   every row done with lamS 0 is the mirror loss alone; the scratch of a term that is off stays NaN-filled (head_partials too, wherever
   the call is one of the single-option calls).
5. Batch edges: fused B in {1, 63, 64, 65, 200}; layer paths B in {1, 31, 255, 256, 257} (the loss block has 256 rows).
6. Both staging forms of the fused head: XBot-L's actor tile has room for the head's 9 600 bytes of LDS, the one-action 768-256-128 actor
   has not (both confirmed with the host's arithmetic, and both accepted by fused_supported).  The launch helper picks the form from the
   room alone, so no shape runs both; each is held to the reference.
7. Misuse is refused with HGYM_E_BADARG and nothing written; the two old entry points' pinned refusals are still there."""
import ctypes as C

import numpy as np
import pytest
import torch

import mirror_smooth_common as MS
import smoothness_common as S
import update_options_common as U
import test_update_options_gpu as G
import test_smoothness_gpu as SG
from hgym import _lib as L

pytestmark = pytest.mark.gpu

O = U.Options
FUSED = [O("bf16-fused", act, "scalar", vu, False, False, sh) for act in (None, U.TANH) for vu in (False, True) for sh in (False, True)]
LAYER = [O(p, act, "scalar", False, False, False, False) for p in ("f32-layer", "bf16-layer") for act in (None, U.TANH)]
EXTRA = [O("bf16-fused", None, "log", False, False, False, True), O("bf16-fused", None, "scalar", False, True, False, True),
         O("bf16-fused", U.TANH, "log", True, True, True, False), O("f32-layer", None, "scalar", True, False, True, False),
         O("bf16-layer", None, "log", True, True, True, False)]
CASES = FUSED + LAYER + EXTRA
ALONE = [O(p, None, "scalar", False, False, False, p == "bf16-fused") for p in U.PATHS]
STEP = SG.STEP
LAMS = (MS.LAM_T, MS.LAM_S)
_NETS = {}


def _net(opts, max_batch=None):
    """G._net's NetBuffers at the suite's max_batch; another max_batch (the batch edges) or the tight fused shape: one of this file's own."""
    if max_batch is None and opts.path != MS.TIGHT:
        return G._net(opts)
    from hgym import NetBuffers, make_net_config
    key = (opts.path, opts.activation is not None, opts.std, max_batch)
    if key not in _NETS:
        assert not opts.aux and not opts.norm
        no, npv, A, ah, ch = U.SHAPES[opts.path]["net"]
        cfg = make_net_config(no, npv, A, ah, ch, "f32" if opts.path == "f32-layer" else "bf16", max_batch or 128, activation=opts.activation,
                              fused_activation=opts.path in ("bf16-fused", MS.TIGHT), noise_std_type=opts.std)
        _NETS[key] = NetBuffers(cfg, "cuda", learning_rate=G.LR)
        assert (_NETS[key].shadow_ld(0) > 0) == (opts.path in ("bf16-fused", MS.TIGHT))
    net = _NETS[key]
    for t in (net.adam_m, net.adam_v, net.opt_state, net.grads_ext):
        t.zero_()
    net.opt_state[L.OPT_LR] = G.LR
    return net


def _tables(case):
    return (torch.tensor(case["spec"].act_src, dtype=torch.int32, device="cuda"), torch.tensor(case["spec"].act_sign, dtype=torch.float32, device="cuda"))


def _call(net, opts, case, ppo, shadow, fn, lam=LAMS, weight=None, rows=None):
    """One gradient call on the case + the unfold.  fn: "both" hgym_ppo_grad_smooth_mirror, "smooth" hgym_ppo_grad_smooth, "grad"
    hgym_ppo_grad (the mirror fields are named whenever ppo.mirror_coef > 0).  Every scratch is NaN-filled and longer than the minibatch
    needs.  -> dict(msums, ssums on the host; mt, tn, ts, pr, hp the device scratch)."""
    import hgym
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:
        sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(torch.bfloat16).cuda().contiguous()
        kw = dict(obs_bf16=sh(case["cols"][0], net.shadow_ld(0)), priv_bf16=sh(case["cols"][1], net.shadow_ld(1)))
    no, A, B = cols[0].shape[1], cols[2].shape[1], case["B"]
    rows = rows or (B + 31)
    ld = hgym.smooth_ld(no)
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    mt, tn, ts, pr = nan(rows * A), nan(rows * A), nan(rows * A), nan(rows * ld)
    hp = nan(hgym.smooth_mirror_partials(B) + 4)
    msums, ssums = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    idx = case["idx"].cuda()
    nxt, w = torch.empty(B, dtype=torch.int64, device="cuda"), torch.empty(B, device="cuda")
    hgym.smooth_pairs(idx, torch.from_numpy(case["dones"]).cuda(), case["N"], nxt, w)
    if weight is not None:
        w.copy_(weight)
    if ppo.mirror_coef > 0.0 or fn == "both":
        kw.update(pair_idx=case["pair"].cuda(), mirror=_tables(case) + (mt, msums))
    net.opt_state[L.OPT_KL_SUM:L.OPT_MINIBATCHES + 1] = 0.0
    net.opt_state[L.OPT_KL_LAST:L.OPT_AUX_SUM + 1] = 0.0
    net.opt_state[L.OPT_STEP] = float(STEP)
    batch = hgym.make_batch(*cols, idx, **kw)
    sm = hgym.make_smooth(lam[0], lam[1], next_idx=nxt, next_weight=w, noise_std=torch.from_numpy(case["noise_std"]).cuda(), seed=S.SEED,
                          target_next=tn, target_near=ts, rows=pr, sums=ssums)
    if fn == "both":
        net.ppo_grad_smooth_mirror(ppo, batch, sm, hp[:hgym.smooth_mirror_partials(B)])
    elif fn == "smooth":
        net.ppo_grad_smooth(ppo, batch, sm)
    else:
        net.ppo_grad(ppo, batch)
    if opts.norm:
        net.norm_unfold_grad()
    torch.cuda.synchronize()
    return dict(msums=msums.cpu(), ssums=ssums.cpu(), mt=mt, tn=tn, ts=ts, pr=pr.view(rows, ld), hp=hp, B=B, A=A, no=no)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check(opts, case, shadow, net=None):
    """Items 1, 2 and 3 on one case: four calls on the same inputs and the same OPT_STEP."""
    net = net or _net(opts)
    G._load(net, opts, case)
    off, on = G._ppo(opts, case), G._ppo(opts, case, mirror_coef=MS.COEF)
    _call(net, opts, case, off, shadow, "grad")
    g0, o0 = net.grads_ext.clone(), net.opt_state.clone()
    m1 = _call(net, opts, case, on, shadow, "grad")                 # the mirror loss alone
    s1 = _call(net, opts, case, off, shadow, "smooth")              # the regulariser alone
    r = _call(net, opts, case, on, shadow, "both")
    assert torch.isfinite(net.grads_ext).all()
    B, A, no = r["B"], r["A"], r["no"]
    for name in ("mt", "tn", "ts"):      # each pre-pass wrote the minibatch's rows, no more
        assert torch.isfinite(r[name][:B * A]).all() and torch.isnan(r[name][B * A:]).all(), name
    assert torch.isfinite(r["pr"][:B]).all() and torch.isnan(r["pr"][B:]).all() and bool((r["pr"][:B, no:] == 0).all())
    nhp = 4 * ((B + 63) // 64)
    blocks = (B + 63) // 64 if opts.path in ("bf16-fused", MS.TIGHT) else 1      # (a loss block of the layer paths covers 256 padded rows: at least one)
    assert torch.isnan(r["hp"][nhp:]).all() and torch.isfinite(r["hp"][:4 * blocks].view(-1, 4)[:, :2]).all()
    near = r["pr"][:B, :no].cpu()
    assert torch.equal(_bits(near), _bits(s1["pr"][:B, :no].cpu()))      # the same OPT_STEP: the same perturbation as the single-option call
    ref = MS.reference(case, near=near)
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    what = "mirror + smooth %s" % U.case_id(opts)
    SG._hold("%s: gradient vs float64 reference" % what, opts, U.errors(opts, got, ref), U.bar_of(opts))
    SG._hold("%s: loss sums" % what, opts, U.sum_errors(opts, G._sums(net), ref), U.SUM_TOL[opts.path])
    tol = U.SUM_TOL[opts.path]
    for name, g, x in (("mirror_sums[0]", float(r["msums"][0]), ref["mirror"]), ("sums[0]", float(r["ssums"][0]), ref["smooth"][0]),
                       ("sums[1]", float(r["ssums"][1]), ref["smooth"][1])):
        if x == 0.0:      # (B = 1: the one row is done)
            assert g == 0.0, name
            continue
        err = abs(g - x) / x
        print("    %-15s %.6e vs %.6e: rel %.3e (bar %.1e)" % (name, g, x, err, tol))
        assert err <= tol, name
    assert float(r["msums"][1]) == 1.0 and float(r["ssums"][2]) == ref["smooth"][2] and float(r["ssums"][3]) == 1.0
    # 2. each term's sums, bit for bit the single-option call's
    assert torch.equal(_bits(r["msums"]), _bits(m1["msums"])), (r["msums"], m1["msums"])
    assert torch.equal(_bits(r["ssums"]), _bits(s1["ssums"])), (r["ssums"], s1["ssums"])
    # 3. everything but the actor's gradient
    SG._others_keep_their_bits(net, g0, o0)
    return net, on, r


# ---------------------------------------------------------------------------------------------- 1. - 3.
@pytest.mark.parametrize("opts", CASES, ids=[U.case_id(o) for o in CASES])
def test_gradient_and_sums_of_every_instantiation(opts):
    case = MS.case_of(opts)
    S.check_mask(case)
    net, ppo, r = _check(opts, case, opts.shadow)
    if opts.shadow:      # the bf16 shadow rows and the fp32 rows give the same bits
        ext = net.grads_ext.clone()
        r2 = _call(net, opts, case, ppo, False, "both")
        assert torch.equal(_bits(ext), _bits(net.grads_ext))
        assert torch.equal(_bits(r["msums"]), _bits(r2["msums"])) and torch.equal(_bits(r["ssums"]), _bits(r2["ssums"]))


@pytest.mark.parametrize("term", ["temporal", "spatial"])
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_one_smoothness_term_beside_the_mirror_loss(opts, term):
    """The mirror loss with ONE of the two terms: the other's scratch stays NaN-filled, its sum 0, the gradient holds the reference."""
    case = MS.case_of(opts)
    lam = (MS.LAM_T, 0.0) if term == "temporal" else (0.0, MS.LAM_S)
    net = _net(opts)
    G._load(net, opts, case)
    ppo = G._ppo(opts, case, mirror_coef=MS.COEF)
    r = _call(net, opts, case, ppo, opts.shadow, "both", lam=lam)
    B, A, no = r["B"], r["A"], r["no"]
    near = None
    if term == "temporal":
        assert torch.isnan(r["ts"]).all() and torch.isnan(r["pr"]).all() and torch.isfinite(r["tn"][:B * A]).all()
        assert float(r["ssums"][1]) == 0.0 and float(r["ssums"][0]) > 0.0
    else:
        assert torch.isnan(r["tn"]).all() and torch.isfinite(r["ts"][:B * A]).all()
        assert float(r["ssums"][0]) == 0.0 and float(r["ssums"][1]) > 0.0
        near = r["pr"][:B, :no].cpu()
    ref = MS.reference(case, lam_t=lam[0], lam_s=lam[1], near=near)
    got = {k: v.cpu() for k, v in net.grad_views().items()}
    SG._hold("mirror + %s term %s" % (term, U.case_id(opts)), opts, U.errors(opts, got, ref), U.bar_of(opts))
    assert abs(float(r["msums"][0]) - ref["mirror"]) <= U.SUM_TOL[opts.path] * ref["mirror"]
    assert float(r["ssums"][2]) == ref["smooth"][2] and float(r["ssums"][3]) == 1.0


# ---------------------------------------------------------------------------------------------- 4. degenerate forms
DEGENERATE = ALONE + [FUSED[5]]


@pytest.mark.parametrize("opts", DEGENERATE, ids=[U.case_id(o) for o in DEGENERATE])
def test_degenerate_forms_are_the_single_option_calls(opts):
    case = MS.case_of(opts)
    net = _net(opts)
    G._load(net, opts, case)
    off, on = G._ppo(opts, case), G._ppo(opts, case, mirror_coef=MS.COEF)
    state = lambda: (net.grads_ext.clone(), net.opt_state.clone())
    same = lambda a: torch.equal(_bits(a[0]), _bits(net.grads_ext)) and torch.equal(_bits(a[1]), _bits(net.opt_state))
    # mirror_coef 0: hgym_ppo_grad_smooth -- head_partials and the mirror target are not looked at
    s1 = _call(net, opts, case, off, opts.shadow, "smooth")
    a = state()
    r = _call(net, opts, case, off, opts.shadow, "both")
    assert same(a) and torch.equal(_bits(r["ssums"]), _bits(s1["ssums"]))
    assert torch.isnan(r["hp"]).all() and torch.isnan(r["mt"]).all() and float(r["msums"].abs().sum()) == 0.0
    for k in ("tn", "ts", "pr"):
        assert torch.equal(_bits(r[k]), _bits(s1[k])), k
    # both smoothness coefficients 0: hgym_ppo_grad with the mirror loss -- no smoothness scratch is written
    m1 = _call(net, opts, case, on, opts.shadow, "grad")
    b = state()
    r = _call(net, opts, case, on, opts.shadow, "both", lam=(0.0, 0.0))
    assert same(b) and torch.equal(_bits(r["msums"]), _bits(m1["msums"])) and torch.equal(_bits(r["mt"]), _bits(m1["mt"]))
    assert float(r["ssums"].abs().sum()) == 0.0
    for k in ("hp", "tn", "ts", "pr"):
        assert torch.isnan(r[k]).all(), k
    # all terms' code runs, lamS 0 and every row done: the temporal term weighs nothing -- the mirror loss alone
    r = _call(net, opts, case, on, opts.shadow, "both", lam=(MS.LAM_T, 0.0), weight=torch.zeros(case["B"], device="cuda"))
    assert torch.equal(_bits(b[0]), _bits(net.grads_ext))
    for slot in SG.OPT_KEPT + (L.OPT_GRAD_SQNORM,):
        assert float(b[1][slot]) == float(net.opt_state[slot]), slot
    assert torch.equal(_bits(r["msums"]), _bits(m1["msums"]))
    assert float(r["ssums"][0]) == 0.0 and float(r["ssums"][2]) == 0.0 and float(r["ssums"][3]) == 1.0
    assert torch.isnan(r["ts"]).all() and torch.isnan(r["pr"]).all()      # the spatial term is off: its scratch is not written


# ---------------------------------------------------------------------------------------------- 5. batch edges
@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
def test_fused_batch_edges(B):
    opts = O("bf16-fused", None, "scalar", False, False, False, True)
    big = B > 97
    case = MS.make_case(opts, seed=60 + B, B=B, layout=(21, 10) if big else None)
    _check(opts, case, True, net=_net(opts, 256) if big else None)


@pytest.mark.parametrize("B", [1, 31, 255, 256, 257])
@pytest.mark.parametrize("path", ["f32-layer", "bf16-layer"])
def test_layer_batch_edges(path, B):
    opts = O(path, None, "scalar", True, False, False, False)      # (unclipped: one row's d V is never 0, the last critic bias's metric is defined)
    big = B > 31
    case = MS.make_case(opts, seed=80 + B, B=B, layout=(27, 10) if big else None)
    _check(opts, case, False, net=_net(opts, 320) if big else None)


# ---------------------------------------------------------------------------------------------- 6. both staging forms
def test_both_staging_forms():
    import test_fused_shapes as FS
    xbot, tight = U.SHAPES["bf16-fused"]["net"], U.SHAPES[MS.TIGHT]["net"]
    room = lambda net: MS.FB_LDS_LIMIT - FS.fb_lds_bytes(net[3], net[2])
    print("room behind the actor's tile: XBot-L %d bytes, %s with %d action %d bytes; the head stages %d" %
          (room(xbot), tight[3], tight[2], room(tight), MS.HEAD_LDS))
    assert room(xbot) >= MS.HEAD_LDS and 0 <= room(tight) < MS.HEAD_LDS
    assert FS._fused(xbot[3], xbot[4], xbot[2]) and FS._fused(tight[3], tight[4], tight[2])      # fused_supported() takes both
    for act in (None, U.TANH):
        opts = O(MS.TIGHT, act, "scalar", False, False, False, True)
        case = MS.make_case(opts, seed=300 + (act is not None))
        S.check_mask(case)
        net, ppo, r = _check(opts, case, True)
        ext = net.grads_ext.clone()
        _call(net, opts, case, ppo, False, "both")
        assert torch.equal(_bits(ext), _bits(net.grads_ext))


# ---------------------------------------------------------------------------------------------- 7. misuse
@pytest.mark.parametrize("opts", ALONE, ids=[U.case_id(o) for o in ALONE])
def test_misuse_is_refused(opts):
    import hgym
    case = MS.case_of(opts)
    net = _net(opts)
    G._load(net, opts, case)
    cols = [t.cuda().contiguous() for t in case["cols"]]
    no, A, B = cols[0].shape[1], cols[2].shape[1], case["B"]
    ld = hgym.smooth_ld(no)
    mt, tn, ts, pr = (torch.zeros(n + 4, device="cuda") for n in (128 * A, 128 * A, 128 * A, 128 * ld))
    nhp = hgym.smooth_mirror_partials(B)
    hp = torch.zeros(nhp + 4, device="cuda")
    msums, sums = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    idx, nxt, w, pair = case["idx"].cuda(), case["nxt"].cuda(), case["weight"].cuda(), case["pair"].cuda()
    ns = torch.from_numpy(case["noise_std"]).cuda()
    tables = _tables(case)
    good_batch = lambda: hgym.make_batch(*cols, idx, pair_idx=pair, mirror=tables + (mt, msums))
    net.grads_ext.fill_(7.0)
    torch.cuda.synchronize()

    def good(lt=MS.LAM_T, ls=MS.LAM_S):
        sm = L.Smooth()
        sm.temporal_coef, sm.spatial_coef, sm.seed = lt, ls, 5
        sm.next_idx, sm.next_weight, sm.noise_std = L.i64ptr(nxt), L.fptr(w), L.fptr(ns)
        sm.target_next, sm.target_near, sm.rows, sm.sums = L.fptr(tn), L.fptr(ts), L.fptr(pr), L.f64ptr(sums)
        return sm

    def rc(sm, ppo=None, b=None, p=hp, n=nhp):
        ppo = ppo or G._ppo(opts, case, mirror_coef=MS.COEF)
        b = b or good_batch()
        ptr = p if p is None or not isinstance(p, torch.Tensor) else L.fptr(p)
        return int(L.lib.hgym_ppo_grad_smooth_mirror(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(b), C.byref(sm), ptr, n, net.stream()))
    err = lambda: L.lib.hgym_last_error()
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert rc(good(lt=bad)) == -1 and b"temporal_coef" in err()
        assert rc(good(ls=bad)) == -1 and b"spatial_coef" in err()
        assert rc(good(), ppo=G._ppo(opts, case, mirror_coef=bad)) == -1 and b"mirror_coef" in err()
    for field in ("next_idx", "next_weight", "noise_std", "target_next", "target_near", "rows", "sums"):
        sm = good()
        setattr(sm, field, None)
        assert rc(sm) == -1, field
    for field, t in (("target_next", tn), ("target_near", ts), ("rows", pr)):
        sm = good()
        setattr(sm, field, C.cast(t.data_ptr() + 4, L.c_float_p))      # not 16-byte aligned
        assert rc(sm) == -1 and b"16-byte" in err(), field
    for field in ("pair_idx", "mirror_act_src", "mirror_act_sign", "mirror_target", "mirror_sums"):
        b = good_batch()
        setattr(b, field, None)
        assert rc(good(), b=b) == -1 and b"mirror" in err(), field
    b = good_batch()
    b.mirror_target = C.cast(mt.data_ptr() + 4, L.c_float_p)
    assert rc(good(), b=b) == -1 and b"16-byte" in err()
    assert rc(good(), p=None) == -1 and b"head_partials" in err()
    assert rc(good(), p=C.cast(hp.data_ptr() + 4, L.c_float_p)) == -1 and b"16-byte" in err()
    assert rc(good(), n=nhp - 1) == -1 and b"head_partials_len" in err()
    two = G._ppo(opts, case, mirror_coef=MS.COEF)
    two.world_size = 2
    assert rc(good(), ppo=two) == -1 and b"world_size" in err()
    # the two pinned refusals of the old entry points are still there
    old = lambda sm, ppo: int(L.lib.hgym_ppo_grad_smooth(C.byref(net.cfg), C.byref(ppo), C.byref(net.struct), C.byref(good_batch()), C.byref(sm), net.stream()))
    assert old(good(), G._ppo(opts, case, mirror_coef=MS.COEF)) == -1 and b"mirror_coef" in err()
    from humanoid.algo.ppo import smoothness as SM
    with pytest.raises(ValueError, match="symmetry"):
        SM.check_setup(symmetry=object())
    torch.cuda.synchronize()
    assert bool((net.grads_ext == 7.0).all()) and float(sums.sum()) == 0.0 and float(msums.sum()) == 0.0      # nothing was launched
    for t in (mt, tn, ts, pr, hp):
        assert float(t.abs().sum()) == 0.0
    # head_partials is not looked at where the call is a single-option call
    assert rc(good(), ppo=G._ppo(opts, case), p=None, n=0) == 0
    assert rc(good(lt=0.0, ls=0.0), p=None, n=0) == 0
    # a term that is off needs none of its pointers
    sm = good(ls=0.0)
    sm.noise_std, sm.target_near, sm.rows = None, None, None
    assert rc(sm) == 0
    sm = good(lt=0.0)
    sm.next_idx, sm.next_weight, sm.target_next = None, None, None
    assert rc(sm) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads_ext).all() and float(sums[3]) == 3.0 and float(msums[1]) == 3.0
