"""-m gpu: the fused bf16 update (mlp_fb_kernel / mlp_fb_act_kernel -> dw_kernel_rs with the loss-scalar workgroup -> reduce_slabs_kernel)
at every edge of the batch dimension, against the float64 oracle on bf16-rounded operands (oracle/ppo_oracle.py:ppo_loss_and_grads with
quant = bf16 round-to-nearest-even, as in tests/test_fused_shapes_gpu.py).

The sizes, the plan they are derived from and the spotlit inputs are tests/fused_batch_common.py's; tests/test_fused_batch_edges.py checks
on the host that the sizes reach every class of the plan and that the rows under test carry at least ten bars of every tensor.

(a) XBot-L widths, every B of BATCHES, every spot: gradient per tensor and loss sums, from fp32 rows and from the bf16 shadows (the
    gathered first-layer products of dw_kernel_rs), the two bit-identical.
(b) the reduced list on the other kernels of the family: fb_body<1> (g1), the scalar loss branch (A = 10), mlp_fb_act_kernel (Tanh), the
    unclipped value loss, and the trunk with a fused denoiser head (twelve products in one launch).
(c) a workspace that held a larger minibatch gives the bits of a fresh one.
(d) hgym_ppo_grad_part 0 then 1 gives the bits of hgym_ppo_grad.

Every storage row outside the index list is NaN, and the gradient buffer is NaN before each call."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16_report as BR
import fused_batch_common as FB
from hgym import _lib as L

pytestmark = pytest.mark.gpu

REDUCED_MAX_BATCH = 3136        # 49 tiles: the largest B of FB.REDUCED
SUMS = slice(L.OPT_KL_SUM, L.OPT_GRAD_SQNORM)      # KL sum, surrogate, value, entropy, (grad norm, minibatches,) last KL
_NETS = {}


def _net(key, max_batch, **kw):
    """One NetBuffers per network shape, shared by the cases of this module (the parameters are FB.make_params' and never stepped)."""
    if key not in _NETS:
        _NETS[key] = _fresh(key if key in FB.SHAPES else "xbotl", max_batch, **kw)
    return _NETS[key]


def _fresh(shape, max_batch, head=None, **kw):
    from hgym import NetBuffers, make_net_config
    no, npv, A, ah, ch = FB.SHAPES[shape]
    net = NetBuffers(make_net_config(no, npv, A, ah, ch, "bf16", max_batch, **kw), "cuda", learning_rate=1e-3)
    assert net.shadow_ld(0) > 0 and net.shadow_ld(1) > 0          # the fused path: no case passes on another kernel
    sd = dict(zip([k for k in net.views if not k.startswith("denoiser")], FB.make_params(shape).tensors()))
    if head is not None:
        for l, (W, b) in enumerate(head):
            sd["denoiser.%d.weight" % (2 * l)], sd["denoiser.%d.bias" % (2 * l)] = W, b
    assert list(sd) == list(net.views)
    net.load_state_dict(sd)
    return net


def _device_batch(net, case, shadow):
    from hgym import make_batch
    cols = [t.cuda().contiguous() for t in case["cols"]]
    kw = {}
    if shadow:      # selected rows: the rounded row, pad columns zero; every other row NaN
        for key, x, which in (("obs_bf16", case["cols"][0], 0), ("priv_bf16", case["cols"][1], 1)):
            s = torch.full((case["S"], net.shadow_ld(which)), float("nan"), dtype=torch.bfloat16)
            s[case["idx"]] = 0.0
            s[case["idx"], :x.shape[1]] = x[case["idx"]].to(torch.bfloat16)
            kw[key] = s.cuda().contiguous()
    idx = case["idx"].cuda()
    return make_batch(*cols, idx, **kw), (cols, idx, kw)        # (make_batch takes addresses: the caller keeps every tensor alive)


def _call(net, ppo, batch, parts=False):
    """One gradient on a NaN-filled buffer and zeroed sums -> (grads_ext, opt_state), on the device."""
    net.opt_state[L.OPT_KL_SUM:L.OPT_AUX_SUM + 1] = 0.0
    net.grads_ext.fill_(float("nan"))
    if parts:
        net.ppo_grad_part(ppo, batch, 0)
        net.ppo_grad_part(ppo, batch, 1)
    else:
        net.ppo_grad(ppo, batch)
    torch.cuda.synchronize()
    return net.grads_ext.clone(), net.opt_state.clone()


def _same_bits(what, a, b):
    """(grads_ext, opt_state) pairs: gradient, KL slot and loss sums bit for bit; the squared norm (fp64 atomics) to rounding."""
    (ga, oa), (gb, ob) = a, b
    assert torch.isfinite(ga).all() and torch.isfinite(gb).all(), what
    diff = float((ga.double() - gb.double()).abs().max())
    BR.check(what + ": max |difference| of the gradients", diff, 0.0)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), what
    assert torch.equal(oa[SUMS], ob[SUMS]) and torch.equal(oa[L.OPT_AUX_SUM], ob[L.OPT_AUX_SUM]), (what, oa, ob)
    np.testing.assert_allclose(float(oa[L.OPT_GRAD_SQNORM]), float(ob[L.OPT_GRAD_SQNORM]), rtol=1e-12)


def _check_scalars(what, case, want, opt, grads_ext, P_):
    """The loss sums ppo_scalars_block leaves in opt_state (+= sum / B on zeroed slots), at tests/test_fused_shapes_gpu.py's bounds for
    the KL and the value loss.  The entropy is a function of std alone (fp32 logs of 12 numbers: 1e-4).  The surrogate is a signed sum
    that cancels, so it is held against the size of its terms: the kernels' log-probability differs from the oracle's by the bf16 error
    of mu, sum_j (a - mu)_j / sigma_j^2 * dmu_j with dmu <= 2e-3 of the output scale (the forward bar) -- a few 1e-3 per row, so
    1e-2 of mean |term|."""
    opt = opt.cpu()
    B = case["B"]
    assert float(opt[L.OPT_MINIBATCHES]) == 1.0
    np.testing.assert_allclose(float(opt[L.OPT_KL_LAST]), float(want["kl"]), rtol=2e-2, atol=1e-4, err_msg=what)
    np.testing.assert_allclose(float(opt[L.OPT_KL_SUM]), float(want["kl"]), rtol=2e-2, atol=1e-4, err_msg=what)
    assert float(grads_ext[P_]) == float(np.float32(float(opt[L.OPT_KL_LAST]))), what
    np.testing.assert_allclose(float(opt[L.OPT_VALUE_SUM]), float(want["value_loss"]), rtol=1e-2, err_msg=what)
    np.testing.assert_allclose(float(opt[L.OPT_ENTROPY_SUM]), float(want["entropy"]), rtol=1e-4, err_msg=what)
    sel = [t[case["idx"]].double() for t in case["cols"]]
    ratio = torch.exp(want["logp"] - sel[6])
    terms = torch.max(-sel[4] * ratio, -sel[4] * ratio.clamp(0.8, 1.2))
    assert abs(float(terms.mean()) - float(want["surrogate"])) < 1e-12 * max(1.0, float(terms.abs().mean()))
    err = abs(float(opt[L.OPT_SURROGATE_SUM]) - float(want["surrogate"])) / float(terms.abs().mean())
    BR.check(what + ": surrogate sum, error / mean |term|", err, 1e-2)


def _check_case(what, net, case, want, bar, ppo, extra=None):
    """fp32 rows and bf16 shadows: bit-identical, and the fp32-row result against the oracle tensor by tensor.  extra(gv, opt) -> more
    {tensor: error} (the auxiliary head's)."""
    res = {}
    for shadow in (False, True):
        batch, keep = _device_batch(net, case, shadow)
        res[shadow] = _call(net, ppo, batch)
        del batch, keep
    _same_bits(what + ", bf16 shadows vs fp32 rows", res[True], res[False])
    grads_ext, opt = res[False]
    base = net.params.data_ptr()
    got = {k: grads_ext[(v.data_ptr() - base) // 4:][:v.numel()].view_as(v).cpu() for k, v in net.views.items()}
    errs = FB.tensor_errors([got[k] for k in FB.NAMES], want["grads"].tensors())
    if extra is not None:
        errs.update(extra(got, opt.cpu()))
    worst = max(errs, key=errs.get)
    print("%s: %s" % (what, ", ".join("%s %.2e" % (k, e) for k, e in errs.items())))
    BR.check("%s vs bf16-operand oracle (worst tensor: %s)" % (what, worst), errs[worst], bar)
    _check_scalars(what, case, want, opt, grads_ext, net.P)
    return errs


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("B", FB.BATCHES)
def test_gradient_at_every_batch_edge(B):
    """XBot-L widths, one net for every B: hgym_ppo_grad on the spotlit minibatch of each spot that exists at B."""
    from hgym import make_ppo_config
    net = _net("xbotl", FB.MAX_BATCH)
    pl = FB.plan(B)
    for spot in FB.spots_of(B):
        case = FB.make_case(B, spot, 1000 + B)
        want = FB.oracle_grad(case)
        what = "fused batch edge B = %d (%d tiles, steps %s), spot %s (%d rows x %.1f)" % (
            B, pl["tiles"], ",".join(str(n) for n in pl["nsteps"]), spot, len(case["spot_pos"]), case["factor"])
        _check_case(what, net, case, want, FB.bar_for(B), make_ppo_config())


# ------------------------------------------------------------------------------------------------ (b)
def _variant_net(variant, monkeypatch):
    from hgym import make_net_config
    if variant in ("g1", "a10"):
        return _net(variant, REDUCED_MAX_BATCH)
    if variant == "tanh":
        return _net("tanh", REDUCED_MAX_BATCH, activation=nn.Tanh(), fused_activation=True)
    if variant == "unclipped":
        return _net("xbotl", FB.MAX_BATCH)
    hidden, out, off, _ = FB.AUX_HEAD
    no, npv, A, ah, ch = FB.SHAPES["xbotl"]
    kw = dict(aux_hidden=hidden, aux_out=out, aux_target_offset=off)
    cfg = make_net_config(no, npv, A, ah, ch, "bf16", REDUCED_MAX_BATCH, **kw)
    ws = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
    monkeypatch.setenv("HGYM_NO_FUSED_AUX", "1")
    ws_generic = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
    monkeypatch.delenv("HGYM_NO_FUSED_AUX")
    assert ws != ws_generic                         # the head kept its fused layout: the third grid row of the same launches
    return _net("aux", REDUCED_MAX_BATCH, head=FB.make_head(tuple(hidden), out), **kw)


@pytest.mark.parametrize("variant", FB.VARIANTS)
def test_reduced_list_on_the_other_kernels(variant, monkeypatch):
    """FB.REDUCED with the tail spot: g1 and a10 at tests/test_fused_shapes_gpu.py's bar, Tanh (restated-activation reference) and the
    unclipped value loss at tests/test_fused_activations_gpu.py's (5e-3 each, here on every tensor as a plain rel-L2), the denoiser head
    against mlp_backward of its MSE at test_aux_head_gradient_vs_oracle's (5e-3, loss rtol 1e-2)."""
    from hgym import make_ppo_config
    import test_fused_shapes_gpu as FS
    assert FS.AUX_CASES["fused"][:2] == FB.AUX_HEAD[:2] and FS.ROWS["g1"][:3] == tuple(FB.SHAPES["g1"][i] for i in (3, 4, 2))
    assert FS.ROWS["a10"][:3] == tuple(FB.SHAPES["a10"][i] for i in (3, 4, 2))
    net = _variant_net(variant, monkeypatch)
    for B in FB.REDUCED:
        case, kw, head = FB.variant_case(variant, B)
        want = FB.oracle_grad(case, **kw)
        ppo = make_ppo_config(clipped_value_loss=variant != "unclipped", aux_coef=head[3] if head else 0.0)
        extra = None
        if head is not None:
            hidden, out, off, coef = head
            hg, mse = FB.oracle_head_grad(case, FB.make_head(tuple(hidden), out), off, out, coef)

            def extra(got, opt, hg=hg, mse=mse):
                np.testing.assert_allclose(float(opt[L.OPT_AUX_SUM]), mse, rtol=1e-2)
                names = ["denoiser.%d.%s" % (2 * l, k) for l in range(4) for k in ("weight", "bias")]
                return {k: FB.rel_l2(got[k], r) for k, r in zip(names, hg)}
        what = "fused batch edge, %s, B = %d, spot tail (%d rows x %.1f)" % (variant, B, len(case["spot_pos"]), case["factor"])
        _check_case(what, net, case, want, FB.BF16_OPERAND_TOL, ppo, extra)


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("shadow", [False, True], ids=["fp32rows", "shadow"])
def test_stale_workspace_gives_the_bits_of_a_fresh_net(shadow):
    """B = 4161 (66 tiles, every split 17 steps), then 65, 1 and 577 on the same net: each result has the bits a freshly created net
    gives for that call -- padded dZ rows, the slabs of empty splits and partial rows past `tiles` leak nothing from a larger call."""
    from hgym import make_ppo_config
    ppo = make_ppo_config()
    net = _fresh("xbotl", FB.MAX_BATCH)
    for B in (4161, 65, 1, 577):
        case = FB.make_case(B, "tail", 3000 + B)
        batch, keep = _device_batch(net, case, shadow)
        got = _call(net, ppo, batch)
        if B != 4161:
            fresh = _fresh("xbotl", FB.MAX_BATCH)
            _same_bits("stale workspace (after B = 4161 ...) vs fresh net, B = %d, %s" % (B, "bf16 shadows" if shadow else "fp32 rows"),
                       got, _call(fresh, ppo, batch))
            del fresh
        del batch, keep


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("shadow", [False, True], ids=["fp32rows", "shadow"])
def test_gradient_in_two_parts_equals_the_whole(shadow):
    """hgym_ppo_grad_part 0 then 1 at B = 577 (splits of 3,3,3,3,3,3,2 steps, one empty) against hgym_ppo_grad."""
    from hgym import make_ppo_config
    ppo = make_ppo_config()
    net = _net("xbotl", FB.MAX_BATCH)
    case = FB.make_case(577, "tail", 4577)
    batch, keep = _device_batch(net, case, shadow)
    whole = _call(net, ppo, batch)
    parts = _call(net, ppo, batch, parts=True)
    _same_bits("hgym_ppo_grad_part 0, 1 vs hgym_ppo_grad, B = 577, %s" % ("bf16 shadows" if shadow else "fp32 rows"), parts, whole)
