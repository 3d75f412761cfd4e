"""-m gpu: hgym_guide_schedule and hgym_ppo_grad_guide stay inside the caller's buffers (DESIGN.md sections 25 and 33), on
tests/test_guard_bands_gpu.py's twin runs: once on ordinary tensors, once with every pointer carved from a guard_common.Arena at exactly
the size include/hgym.h states; afterwards the bands are clean and the outputs carry the twin's bits.

B = 65: two update tiles, the second with one row.  On the fused path with both forms of the head: XBot-L's actor stages the tile's 64
target rows in LDS; the one-action 768-256-128 actor of mirror_smooth_common.TIGHT gathers no loss input through LDS (its head is not 12
wide) and reads its targets from memory.  Stored rows that idx does not name are 0xFF in every column, the teacher's included.  Sizes: the
count one int64, the coefficient one float, teacher_mu exactly (stored rows, A), sums two doubles."""
import pytest
import torch

import guidance_common as GC
import mirror_smooth_common as MS
import update_options_common as U
import test_guard_bands_gpu as GB
from hgym import _lib as L

pytestmark = pytest.mark.gpu

B = 65
F32, F64, I64, U8, BF16 = torch.float32, torch.float64, torch.int64, torch.uint8, torch.bfloat16
FORMS = [("bf16-fused", "staged"), ("bf16-fused", "unstaged"), ("f32-layer", "layer"), ("bf16-layer", "layer")]


@pytest.mark.parametrize("k", [0, 1, 7])
def test_guide_schedule(k):
    import hgym

    def case(side):
        A = side.A
        count = A.place(torch.tensor([k], dtype=I64))
        coef = A.carve(1, F32)
        hgym.guide_schedule(GC.sched(), count, coef)
        side.verify("the call")
        return dict(count=count, coef=coef)
    GB._pair(case, "hgym_guide_schedule k=%d" % k)


@pytest.mark.parametrize("path,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_guided_update(path, form):
    import hgym
    from hgym import make_batch, make_ppo_config
    tight = form == "unstaged"
    case_opts = U.Options(MS.TIGHT if tight else path, None, "scalar", False, False, False, False)
    case = GC.make_case(case_opts, seed=950 + FORMS.index((path, form)), B=B) if path != "f32-layer" else _small_case(case_opts)
    opts = GB._opts(path)      # (the nets' key: the tight shape rides on the fused path's flag through `net`)
    nets = GB._nets(opts, net=U.SHAPES[MS.TIGHT]["net"] if tight else None)
    A = case["cols"][2].shape[1]
    assert (A == 12) == (form != "unstaged" and path != "f32-layer")
    stored = case["cols"][0].shape[0]
    named = torch.zeros(stored, dtype=torch.bool)
    named[case["idx"]] = True
    shadow = path == "bf16-fused"

    def run(side):
        net, A_, out = side.net, side.A, {}
        GB._fresh(net, opts, case)
        cols = [A_.place(t, skew=4 if i < 2 else 0) for i, t in enumerate(case["cols"])]
        kw = {}
        if shadow:
            sh = lambda x, w: torch.nn.functional.pad(x, (0, w - x.shape[1])).to(BF16)
            kw.update(obs_bf16=A_.place(sh(case["cols"][0], net.shadow_ld(0))), priv_bf16=A_.place(sh(case["cols"][1], net.shadow_ld(1))))
        tmu = A_.place(case["teacher_mu"])
        assert tmu.shape == (stored, A) and tmu.data_ptr() % 16 == 0
        for t in cols + list(kw.values()) + [tmu]:
            t.view(U8).view(stored, -1)[(~named).to(GB.DEV)] = 0xFF
        idx = A_.place(case["idx"])
        count, coef, sums = A_.place(torch.tensor([GC.K], dtype=I64)), A_.carve(1, F32), A_.zeros(2, F64)
        ppo = make_ppo_config(grad_norm_ready=False, aux_coef=0.0, clipped_value_loss=True)
        hgym.guide_schedule(GC.sched(), count, coef)
        side.verify("hgym_guide_schedule")
        net.ppo_grad_guide(ppo, make_batch(*cols, idx, **kw), hgym.make_guide(tmu, coef, sums))
        side.verify("hgym_ppo_grad_guide")
        out["grads_ext"] = net.grads_ext.clone()
        GB._opt_state(net, out, "opt_state after grad")
        out.update(sums=sums, coef=coef, count=count)
        assert float(sums[1]) == 1.0 and float(sums[0]) > 0.0 and float(coef) == GC.coef_at(GC.K) and int(count) == GC.K + 1
        assert torch.isfinite(net.grads_ext).all()
        net.ppo_apply(ppo)
        side.verify("hgym_ppo_apply")
        out.update(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone())
        GB._opt_state(net, out, "opt_state")
        return out
    GB._pair(run, "guided update %s %s B=%d" % (path, form, B), nets=nets)


def _small_case(opts):
    """The small fp32 net's own shape stores 50 rows: 70 hold the 65."""
    c = U.make_case(opts, S=70, B=B, seed=953)
    g = torch.Generator().manual_seed(GC.TEACHER_SEED + 953)
    mu_t, _, _ = U.forward(opts, U.make_params(opts, g), c["stats"], c["cols"][0], c["cols"][1])
    return dict(c, teacher_params=None, teacher_mu=mu_t.float().contiguous())
