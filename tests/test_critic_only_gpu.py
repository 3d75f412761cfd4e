"""-m gpu: hgym_vf_grad and hgym_bc_vf_grad on the device, on every update path: the fp32 layer-by-layer path, the
fused bf16 path from fp32 rows and from the bf16 shadow, ELU(1) and nn.Tanh().  B in {1, 63, 64, 65, 255, 256, 257} of 320 stored rows.

  1. fused path: the critic region of the gradient equals hgym_ppo_grad's on the same batch, bit for bit
  2. gradient (layer path) and sums (every path) against float64 at the update's bars: fp32 1e-4, bf16 5e-3 relative L2
  3. keep_others: 0 leaves +0.0 outside the critic and SETS the squared norm, 1 leaves planted values and ADDS it
  4. hgym_bc_vf_grad equals hgym_bc_grad followed by hgym_vf_grad(keep_others = 1), bit for bit
  5. every HGYM_E_BADARG case launches nothing
  6. five vf_grad + ppo_apply steps lower the value loss strictly; actor, std and their Adam moments keep their bits"""
import ctypes as C

import numpy as np
import pytest
import torch

import critic_only_common as CO
from hgym import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 1e-3
_NETS = {}
WORST = {}      # path: the worst measured error (printed by the last case of a path)


def _net(name):
    from hgym import NetBuffers, make_net_config
    if name not in _NETS:
        prec, ad, cd, _ = CO.NETS[name]
        cfg = make_net_config(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], prec, CO.STORED, activation=CO.activation(name),
                              fused_activation=name in CO.FUSED)
        _NETS[name] = NetBuffers(cfg, DEV, learning_rate=LR)
    net = _NETS[name]
    for t in (net.adam_m, net.adam_v, net.grads_ext, net.opt_state):
        t.zero_()
    net.opt_state[L.OPT_LR] = LR
    net.load_state_dict(dict(zip(list(net.views), CO.make_params(name).tensors())))
    assert (net.shadow_ld(1) > 0) == (name in CO.FUSED), "%s is not on the path this test is about" % name
    return net


def _shadow(rows, ld):
    """The bf16 shadow of stored rows: the rows rounded, pad columns zero (NaN rows stay NaN: nobody may read them)."""
    s = torch.zeros(rows.shape[0], ld, dtype=torch.bfloat16)
    s[:, :rows.shape[1]] = rows.to(torch.bfloat16)
    return s.to(DEV)


def _tensors(net, case, shadow):
    cols = [t.to(DEV) for t in case["cols"]]
    sh = dict(obs_bf16=_shadow(case["cols"][0], net.shadow_ld(0)), priv_bf16=_shadow(case["cols"][1], net.shadow_ld(1))) if shadow else {}
    return cols, case["target"].to(DEV), case["idx"].to(DEV), sh


def _vf_batch(cols, idx, sh, unclipped=False, with_obs=False):
    from hgym import make_vf_batch
    return make_vf_batch(cols[1], None if unclipped else cols[3], cols[5], idx, priv_bf16=sh.get("priv_bf16"),
                         obs=cols[0] if with_obs else None, obs_bf16=sh.get("obs_bf16") if with_obs else None)


def _vf_cfg(unclipped=False, keep=False):
    from hgym import make_vf_config
    return make_vf_config(CO.CLIP, CO.VALUE_COEF, clipped_value_loss=not unclipped, keep_others=keep)


def _critic_views(net, flat):
    base = net.params.data_ptr()
    return [flat[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v).cpu() for k, v in net.views.items() if k.startswith("critic.")]


def _critic_range(net):
    lo = net.bucket_split
    hi = int(L.lib.hgym_net_param_offset(C.byref(net.cfg), 2))
    assert 12 < lo < hi == net.P
    return lo, hi


FORMS = [(name, shadow, unclipped) for name in CO.FUSED for shadow in (False, True) for unclipped in (False, True)]


# ------------------------------------------------------------------------------------------------ 1. the critic region of hgym_ppo_grad
@pytest.mark.parametrize("B", CO.BATCHES)
@pytest.mark.parametrize("name, shadow, unclipped", FORMS, ids=["%s-%s-%s" % (n, "shadow" if s else "rows", "vu" if u else "clip") for n, s, u in FORMS])
def test_fused_critic_region_equals_ppo_grad(name, shadow, unclipped, B):
    from hgym import make_batch, make_ppo_config
    net, case = _net(name), CO.make_case(name, B)
    cols, _, idx, sh = _tensors(net, case, shadow)
    lo, hi = _critic_range(net)
    ppo = make_ppo_config(clip_param=CO.CLIP, value_loss_coef=CO.VALUE_COEF, clipped_value_loss=not unclipped)
    net.grads_ext.fill_(float("nan"))
    net.ppo_grad(ppo, make_batch(*cols, idx, **sh))
    torch.cuda.synchronize()
    want, want_sum = net.grads_ext[lo:hi].clone(), float(net.opt_state[L.OPT_VALUE_SUM])
    assert torch.isfinite(want).all()
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    net.grads_ext.fill_(float("nan"))
    net.vf_grad(_vf_cfg(unclipped), _vf_batch(cols, idx, sh, unclipped), sums)
    torch.cuda.synchronize()
    got = net.grads_ext[lo:hi]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "%d of %d critic entries differ from hgym_ppo_grad's" % (
        int((got.view(torch.int32) != want.view(torch.int32)).sum()), hi - lo)
    assert float(sums[1]) == 1.0
    np.testing.assert_allclose(float(sums[0]), want_sum, rtol=1e-12)      # the same partials in the same order


# ------------------------------------------------------------------------------------------------ 2. against float64
PATHS = [("ragged", False), ("ragged_tanh", False), ("fused", False), ("fused", True), ("fused_tanh", False), ("fused_tanh", True)]


@pytest.mark.parametrize("unclipped", [False, True], ids=["clip", "vu"])
@pytest.mark.parametrize("B", CO.BATCHES)
@pytest.mark.parametrize("name, shadow", PATHS, ids=["%s-%s" % (n, "shadow" if s else "rows") for n, s in PATHS])
def test_vf_grad_equals_the_float64_reference(name, shadow, B, unclipped):
    net, case = _net(name), CO.make_case(name, B)
    want_loss, want = CO.reference(name, B, unclipped)
    cols, _, idx, sh = _tensors(net, case, shadow)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    net.grads_ext.fill_(float("nan"))
    net.vf_grad(_vf_cfg(unclipped), _vf_batch(cols, idx, sh, unclipped), sums)
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads_ext).all()
    errs = [CO.rel_l2(g, w) for g, w in zip(_critic_views(net, net.grads_ext), want)]
    loss_err = abs(float(sums[0]) - want_loss) / want_loss
    key = "%s %s" % (name, "shadow" if shadow else "rows")
    WORST[key] = tuple(max(x, y) for x, y in zip(WORST.get(key, (0.0, 0.0)), (max(errs), loss_err)))
    print("%s B=%d %s: worst tensor rel-L2 %.3g (tensor %d of 8), loss error %.3g (bar %.3g); path's worst so far %.3g / %.3g" % (
        key, B, "unclipped" if unclipped else "clipped", max(errs), errs.index(max(errs)), loss_err, CO.bar(name), WORST[key][0], WORST[key][1]))
    assert float(sums[1]) == 1.0 and loss_err <= CO.bar(name), (key, B, loss_err)
    assert len(errs) == len(want) and max(errs) <= CO.bar(name), (key, B, errs)
    lo, hi = _critic_range(net)
    sq = float((net.grads_ext[lo:hi].double() ** 2).sum())
    np.testing.assert_allclose(float(net.opt_state[L.OPT_GRAD_SQNORM]), sq, rtol=1e-6, atol=2e-11)


# ------------------------------------------------------------------------------------------------ 3. keep_others
@pytest.mark.parametrize("name, shadow", [("ragged", False), ("fused", False), ("fused_tanh", True)])
def test_keep_others(name, shadow):
    net, case = _net(name), CO.make_case(name, 65)
    cols, _, idx, sh = _tensors(net, case, shadow)
    lo, hi = _critic_range(net)
    keep_slots = [i for i in range(L.OPT_STATE) if i != L.OPT_GRAD_SQNORM]
    net.opt_state[L.OPT_KL_SUM:L.OPT_AUX_SUM + 1] = torch.arange(1, 10, dtype=torch.float64, device=DEV) * 0.37      # anything: it must survive
    before = net.opt_state.clone()
    # 0: +0.0 outside, the norm SET
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    net.grads_ext.fill_(float("nan"))
    net.opt_state[L.OPT_GRAD_SQNORM] = 123.0
    net.vf_grad(_vf_cfg(keep=False), _vf_batch(cols, idx, sh), sums)
    torch.cuda.synchronize()
    bits = net.grads_ext.view(torch.int32)
    assert int(bits[:lo].abs().max()) == 0 and int(bits[hi:].abs().max()) == 0, "std / actor / KL slot are not +0.0"
    assert int((bits[lo:hi] != 0).sum()) > 0.9 * (hi - lo)
    critic, sq0 = net.grads_ext[lo:hi].clone(), float(net.opt_state[L.OPT_GRAD_SQNORM])
    np.testing.assert_allclose(sq0, float((critic.double() ** 2).sum()), rtol=1e-6, atol=2e-11)
    assert torch.equal(net.opt_state[keep_slots], before[keep_slots]), "a slot of opt_state other than GRAD_SQNORM changed"
    # 1: planted values survive bit for bit, the norm ADDED (1.5: a multiple of the slab sum's quantum, so the addition is exact)
    planted = torch.randn(net.P + 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    net.grads_ext.copy_(planted)
    net.opt_state[L.OPT_GRAD_SQNORM] = 1.5
    net.vf_grad(_vf_cfg(keep=True), _vf_batch(cols, idx, sh), sums)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(net.grads_ext[:lo], planted[:lo]) and same(net.grads_ext[hi:], planted[hi:]), "a planted value outside the critic changed"
    assert same(net.grads_ext[lo:hi], critic), "the critic's gradient depends on keep_others"
    assert float(net.opt_state[L.OPT_GRAD_SQNORM]) == 1.5 + sq0
    assert float(sums[1]) == 2.0 and torch.equal(net.opt_state[keep_slots], before[keep_slots])


# ------------------------------------------------------------------------------------------------ 4. the combined cloning call
BC_FORMS = [("ragged", False, "mse"), ("ragged_tanh", False, "huber"), ("fused", False, "mse"), ("fused", True, "huber"), ("fused_tanh", True, "mse")]


@pytest.mark.parametrize("B", CO.BATCHES)
@pytest.mark.parametrize("name, shadow, loss_type", BC_FORMS, ids=["%s-%s-%s" % (n, "shadow" if s else "rows", t) for n, s, t in BC_FORMS])
def test_bc_vf_grad_equals_the_two_calls_in_sequence(name, shadow, loss_type, B):
    from hgym import make_bc_batch, make_bc_config
    net, case = _net(name), CO.make_case(name, B)
    cols, target, idx, sh = _tensors(net, case, shadow)
    bc = make_bc_config(loss_type, 1.0)
    unclipped = loss_type == "huber"
    z = lambda: torch.zeros(2, dtype=torch.float64, device=DEV)
    seq_bc, seq_vf, one_bc, one_vf = z(), z(), z(), z()
    net.grads_ext.fill_(float("nan"))
    net.bc_grad(bc, make_bc_batch(cols[0], idx, sh.get("obs_bf16")), target, seq_bc)
    net.vf_grad(_vf_cfg(unclipped, keep=True), _vf_batch(cols, idx, sh, unclipped), seq_vf)
    torch.cuda.synchronize()
    want, want_sq = net.grads_ext.clone(), float(net.opt_state[L.OPT_GRAD_SQNORM])
    assert torch.isfinite(want).all()
    net.grads_ext.fill_(float("nan"))
    net.opt_state[L.OPT_GRAD_SQNORM] = 77.0
    net.bc_vf_grad(bc, _vf_cfg(unclipped), _vf_batch(cols, idx, sh, unclipped, with_obs=True), target, one_bc, one_vf)
    torch.cuda.synchronize()
    assert torch.equal(net.grads_ext.view(torch.int32), want.view(torch.int32)), "%d entries differ" % int(
        (net.grads_ext.view(torch.int32) != want.view(torch.int32)).sum())
    assert torch.equal(one_bc, seq_bc) and torch.equal(one_vf, seq_vf), (one_bc, seq_bc, one_vf, seq_vf)
    got_sq = float(net.opt_state[L.OPT_GRAD_SQNORM])      # below 128 the slab sum's additions are exact, above they round in arrival order
    assert got_sq == want_sq if want_sq < 128.0 else abs(got_sq - want_sq) <= 1632 * 2.0 ** -53 * want_sq, (got_sq, want_sq)
    lo, _ = _critic_range(net)
    assert int(net.grads_ext.view(torch.int32)[:12].abs().max()) == 0 and int(net.grads_ext.view(torch.int32)[net.P:].abs().max()) == 0
    assert int((net.grads_ext.view(torch.int32)[12:lo] != 0).sum()) > 0.9 * (lo - 12)


# ------------------------------------------------------------------------------------------------ 5. refusals
SENTINEL = -7.25
BADARG = -1      # HGYM_E_BADARG


@pytest.mark.parametrize("name", ["ragged", "fused"])
def test_every_badarg_case_launches_nothing(name):
    from hgym import make_bc_config
    net, case = _net(name), CO.make_case(name, 65)
    cols, target, idx, sh = _tensors(net, case, name in CO.FUSED)
    sums, sums2 = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    net.grads_ext.fill_(SENTINEL)
    opt0, ws0 = net.opt_state.clone(), net.workspace.clone()
    nan, inf = float("nan"), float("inf")
    bc = make_bc_config("mse")

    def cfg(**kw):
        c = _vf_cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def batch(**kw):
        b = _vf_batch(cols, idx, sh, with_obs=True)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    f64, s = L.f64ptr, net.stream()
    big = torch.zeros(CO.STORED + 1, dtype=torch.int64, device=DEV)
    cases = [("NULL sums", cfg(), batch(), None), ("NULL config", None, batch(), sums),
             ("clip NaN", cfg(clip_param=nan), batch(), sums), ("clip negative", cfg(clip_param=-0.1), batch(), sums),
             ("clip inf", cfg(clip_param=inf), batch(), sums), ("coef NaN", cfg(value_coef=nan), batch(), sums),
             ("coef negative", cfg(value_coef=-1.0), batch(), sums), ("coef inf", cfg(value_coef=inf), batch(), sums),
             ("B = 0", cfg(), batch(B=0), sums), ("B > max_batch", cfg(), batch(B=CO.STORED + 1, idx=L.i64ptr(big)), sums),
             ("NULL values, clipped", cfg(), batch(values=None), sums), ("NULL returns", cfg(), batch(returns=None), sums),
             ("NULL priv", cfg(), batch(priv=None), sums), ("NULL idx", cfg(), batch(idx=None), sums),
             ("unclipped = 2", cfg(unclipped=2), batch(), sums), ("keep_others = 2", cfg(keep_others=2), batch(), sums)]
    for what, c, b, sm in cases:
        rc = L.lib.hgym_vf_grad(C.byref(net.cfg), None if c is None else C.byref(c), C.byref(net.struct), C.byref(b), f64(sm), s)
        assert rc == BADARG, "hgym_vf_grad, %s: %d" % (what, rc)
        rc = L.lib.hgym_bc_vf_grad(C.byref(net.cfg), C.byref(bc), None if c is None else C.byref(c), C.byref(net.struct), C.byref(b),
                                   L.fptr(target), f64(sums2), f64(sm), s)
        assert rc == BADARG, "hgym_bc_vf_grad, %s: %d" % (what, rc)
    for what, args in [("NULL target", (bc, None, sums2)), ("NULL bc_sums", (bc, target, None)), ("NULL bc", (None, target, sums2)),
                       ("one block for both sums", (bc, target, sums)), ("bad loss_type", (L.BCConfig(5, 1.0), target, sums2)),
                       ("Huber delta 0", (L.BCConfig(L.BC_HUBER, 0.0), target, sums2))]:
        b_, t_, s_ = args
        rc = L.lib.hgym_bc_vf_grad(C.byref(net.cfg), None if b_ is None else C.byref(b_), C.byref(_vf_cfg()), C.byref(net.struct),
                                   C.byref(batch()), L.fptr(t_), f64(s_), f64(sums), s)
        assert rc == BADARG, "hgym_bc_vf_grad, %s: %d" % (what, rc)
    rc = L.lib.hgym_bc_vf_grad(C.byref(net.cfg), C.byref(bc), C.byref(_vf_cfg()), C.byref(net.struct), C.byref(batch(obs=None)),
                               L.fptr(target), f64(sums2), f64(sums), s)
    assert rc == BADARG
    torch.cuda.synchronize()
    assert bool((net.grads_ext == SENTINEL).all()), "a refused call wrote the gradient buffer"
    assert torch.equal(net.opt_state, opt0) and torch.equal(net.workspace, ws0) and float(sums.abs().sum() + sums2.abs().sum()) == 0.0
    # the unclipped form does not read `values`, nor clip_param
    net.vf_grad(cfg(unclipped=1, clip_param=nan), batch(values=None), sums)
    torch.cuda.synchronize()
    assert float(sums[1]) == 1.0 and torch.isfinite(net.grads_ext).all()


# ------------------------------------------------------------------------------------------------ 6. the critic learns, nothing else moves
@pytest.mark.parametrize("name, shadow", [("ragged", False), ("ragged_tanh", False), ("fused", True), ("fused_tanh", False)])
def test_five_steps_lower_the_value_loss_and_move_the_critic_alone(name, shadow):
    """At the library's default learning rate (NetBuffers' own, 1e-5: XBot-L's train config has the same).  From zero moments Adam's first
    steps are lr * sign(g) in every weight, whatever the gradient's size: at the cases' 1e-3 the 256-wide critic overshoots the fixed
    batch by its fourth step, which says nothing about the gradient."""
    import inspect
    from hgym import NetBuffers, make_ppo_config
    net, case = _net(name), CO.make_case(name, 257)
    lr = inspect.signature(NetBuffers.__init__).parameters["learning_rate"].default
    net.opt_state[L.OPT_LR] = lr
    cols, _, idx, sh = _tensors(net, case, shadow)
    lo, hi = _critic_range(net)
    ppo = make_ppo_config(max_grad_norm=1.0, desired_kl=0.0, adaptive=False, grad_norm_ready=False)
    before = dict(params=net.params.clone(), sigma=net.sigma.clone())
    losses = []
    for _ in range(6):      # the sixth gradient call reports the loss behind the fifth step
        sums = torch.zeros(2, dtype=torch.float64, device=DEV)
        net.vf_grad(_vf_cfg(), _vf_batch(cols, idx, sh), sums)
        losses.append(sums)
        if len(losses) <= 5:
            net.ppo_apply(ppo)
    torch.cuda.synchronize()
    losses = [float(s[0]) for s in losses]
    print("%s: value loss over five steps at lr %g: %s" % (name, lr, ", ".join("%.8g" % v for v in losses)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(net.params[:lo], before["params"][:lo]) and same(net.sigma, before["sigma"]), "std or an actor parameter moved"
    assert not same(net.params[lo:hi], before["params"][lo:hi])
    assert int(net.adam_m[:lo].view(torch.int32).abs().max()) == 0 and int(net.adam_v[:lo].view(torch.int32).abs().max()) == 0
    assert lr == 1e-5 and float(net.opt_state[L.OPT_STEP]) == 5.0 and float(net.opt_state[L.OPT_LR]) == lr
