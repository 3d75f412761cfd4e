"""-m gpu: hgym_vf_grad and hgym_bc_vf_grad stay inside the caller's buffers (DESIGN.md sections 25 and 34), on
tests/test_guard_bands_gpu.py's twin runs: once on ordinary tensors, once with every pointer carved from a guard_common.Arena at exactly
the size include/hgym.h states; afterwards the bands are clean and the outputs carry the twin's bits.

B = 65: two update tiles, the second with one row; one loss block of the layer-by-layer path with 191 padding threads.  The fused path
from fp32 rows and from the bf16 shadow, with the loss inputs staged in LDS (fused_tanh: third width 128) and read from memory (fused);
the layer-by-layer path in fp32 and bf16.  Stored rows that idx does not name are 0xFF in every column.  Sizes: priv exactly (stored rows,
num_priv), values and returns (stored rows,), idx (B,), the shadow (stored rows, hgym_net_shadow_ld), sums two doubles each."""
import pytest
import torch

import critic_only_common as CO
import guard_common as G
import test_guard_bands_gpu as GB
from hgym import _lib as L

pytestmark = pytest.mark.gpu

B = 65
F32, F64, I64, U8, BF16 = torch.float32, torch.float64, torch.int64, torch.uint8, torch.bfloat16
FORMS = [("fused", False), ("fused", True), ("fused_tanh", True), ("ragged", False), ("ragged_tanh", False)]
_NETS = {}


def _nets(name):
    """(twin, guarded net, the guarded net's arena): the guarded net's buffers have exactly the header's sizes."""
    from hgym import NetBuffers, make_net_config
    if name not in _NETS:
        prec, ad, cd, _ = CO.NETS[name]
        cfg = make_net_config(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], prec, CO.STORED, activation=CO.activation(name),
                              fused_activation=name in CO.FUSED)
        arena = G.Arena(GB.DEV, G.net_arena_bytes(cfg))
        _NETS[name] = (NetBuffers(cfg, GB.DEV, learning_rate=GB.LR), G.guard_net(cfg, arena, learning_rate=GB.LR), arena)
    return _NETS[name]


def _fresh(net, name):
    for t in (net.adam_m, net.adam_v, net.grads_ext, net.opt_state, net.workspace):
        t.zero_()
    net.opt_state[L.OPT_LR] = GB.LR
    net.load_state_dict(dict(zip(list(net.views), CO.make_params(name).tensors())))


def _place(side, case, net, shadow, with_obs):
    """The call's inputs on the side's allocator, unnamed rows 0xFF: -> (cols by name, target, idx, shadows by name)."""
    A_ = side.A
    named = torch.zeros(CO.STORED, dtype=torch.bool)
    named[case["idx"]] = True
    cols = dict(priv=A_.place(case["cols"][1], skew=4), values=A_.place(case["cols"][3]), returns=A_.place(case["cols"][5]))
    if with_obs:
        cols["obs"] = A_.place(case["cols"][0], skew=4)
    target = A_.place(case["target"]) if with_obs else None
    sh = {}
    if shadow:
        pad = lambda x, w: torch.nn.functional.pad(x, (0, w - x.shape[1])).to(BF16)
        sh["priv_bf16"] = A_.place(pad(case["cols"][1], net.shadow_ld(1)))
        if with_obs:
            sh["obs_bf16"] = A_.place(pad(case["cols"][0], net.shadow_ld(0)))
    for t in list(cols.values()) + list(sh.values()) + ([target] if with_obs else []):
        t.view(U8).view(CO.STORED, -1)[(~named).to(GB.DEV)] = 0xFF
    return cols, target, A_.place(case["idx"]), sh


@pytest.mark.parametrize("keep", [False, True], ids=["set", "keep"])
@pytest.mark.parametrize("name, shadow", FORMS, ids=["%s-%s" % (n, "shadow" if s else "rows") for n, s in FORMS])
def test_vf_grad(name, shadow, keep):
    from hgym import make_ppo_config, make_vf_batch, make_vf_config
    case = CO.make_case(name, B)

    def run(side):
        net, out = side.net, {}
        _fresh(net, name)
        cols, _, idx, sh = _place(side, case, net, shadow, False)
        sums = side.A.zeros(2, F64)
        if keep:      # planted values outside the critic's region: they must come back
            net.grads_ext.copy_(torch.randn(net.P + 1, generator=torch.Generator().manual_seed(5)).to(GB.DEV))
        net.vf_grad(make_vf_config(CO.CLIP, CO.VALUE_COEF, keep_others=keep), make_vf_batch(cols["priv"], cols["values"], cols["returns"], idx, **sh), sums)
        side.verify("hgym_vf_grad")
        out["grads_ext"] = net.grads_ext.clone()
        GB._opt_state(net, out, "opt_state after grad")
        out["sums"] = sums
        assert float(sums[1]) == 1.0 and float(sums[0]) > 0.0 and torch.isfinite(net.grads_ext).all()
        net.ppo_apply(make_ppo_config(adaptive=False, grad_norm_ready=False))
        side.verify("hgym_ppo_apply")
        out.update(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone())
        GB._opt_state(net, out, "opt_state")
        return out
    GB._pair(run, "critic-only update %s %s keep_others=%d B=%d" % (name, "shadow" if shadow else "rows", keep, B), nets=_nets(name))


@pytest.mark.parametrize("name, shadow", FORMS, ids=["%s-%s" % (n, "shadow" if s else "rows") for n, s in FORMS])
def test_bc_vf_grad(name, shadow):
    from hgym import make_bc_config, make_ppo_config, make_vf_batch, make_vf_config
    case = CO.make_case(name, B)

    def run(side):
        net, out = side.net, {}
        _fresh(net, name)
        cols, target, idx, sh = _place(side, case, net, shadow, True)
        assert target.data_ptr() % 16 == 0
        bc_sums, vf_sums = side.A.zeros(2, F64), side.A.zeros(2, F64)
        net.grads_ext.fill_(float("nan"))
        batch = make_vf_batch(cols["priv"], cols["values"], cols["returns"], idx, priv_bf16=sh.get("priv_bf16"), obs=cols["obs"], obs_bf16=sh.get("obs_bf16"))
        net.bc_vf_grad(make_bc_config("huber", 1.0), make_vf_config(CO.CLIP, CO.VALUE_COEF), batch, target, bc_sums, vf_sums)
        side.verify("hgym_bc_vf_grad")
        out["grads_ext"] = net.grads_ext.clone()
        GB._opt_state(net, out, "opt_state after grad")
        out.update(bc_sums=bc_sums, vf_sums=vf_sums)
        assert float(bc_sums[1]) == 1.0 and float(vf_sums[1]) == 1.0 and float(bc_sums[0]) > 0.0 and float(vf_sums[0]) > 0.0
        assert torch.isfinite(net.grads_ext).all()
        net.ppo_apply(make_ppo_config(adaptive=False, grad_norm_ready=False))
        side.verify("hgym_ppo_apply")
        out.update(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone())
        GB._opt_state(net, out, "opt_state")
        return out
    GB._pair(run, "cloning step with the critic %s %s B=%d" % (name, "shadow" if shadow else "rows", B), nets=_nets(name))
