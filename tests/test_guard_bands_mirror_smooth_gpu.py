"""-m gpu: hgym_ppo_grad_smooth_mirror between guard bands (tests/guard_common.py), with the harness of
tests/test_guard_bands_gpu.py: one unguarded twin, one run whose every buffer is carved at exactly the size include/hgym.h states.

B = 65 (two update tiles, the second with one row; one loss block) on all three paths, and on the fused path in both staging forms of the
head (XBot-L's actor stages its targets in LDS; the one-action 768-256-128 actor of mirror_smooth_common.TIGHT has no room and reads them
from memory).  Stored rows nobody names -- neither idx nor, for the observations, the successor and the partner rows -- are 0xFF.  Sizes:
pair_idx, next_idx, next_weight exactly B; mirror_target, target_next, target_near exactly (B, A); rows exactly (B, num_obs rounded up
to 4); noise_std exactly num_obs; mirror_sums 2 and sums 4 doubles; head_partials exactly 4 * ceil(B / 64) floats.  The bands stay
clean, the outputs carry the twin's bits, every float is finite."""
import pytest
import torch

import guard_common as G
import mirror_smooth_common as MS
import smoothness_common as S
import update_options_common as U
import test_guard_bands_gpu as GB

pytestmark = pytest.mark.gpu

B = 65
F32, F64, I32, U8, BF16 = torch.float32, torch.float64, torch.int32, torch.uint8, torch.bfloat16
FORMS = [("bf16-fused", "staged"), ("bf16-fused", "unstaged"), ("f32-layer", "layer"), ("bf16-layer", "layer")]


@pytest.mark.parametrize("path,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_smooth_mirror_update(path, form):
    import hgym
    from hgym import make_batch, make_ppo_config
    tight = form == "unstaged"
    case_opts = U.Options(MS.TIGHT if tight else path, None, "scalar", False, False, False, False)
    # (the small fp32 net's own layout stores 50 rows: 14 steps of 5 envs hold the 65)
    case = MS.make_case(case_opts, seed=900 + FORMS.index((path, form)), B=B, layout=(14, 5) if path == "f32-layer" else None)
    opts = GB._opts(path)      # (the nets' key: the tight shape rides on the fused path's flag through `net`)
    nets = GB._nets(opts, net=U.SHAPES[MS.TIGHT]["net"] if tight else None)
    no, A = case["cols"][0].shape[1], case["cols"][2].shape[1]
    if path == "bf16-fused":      # the staging form follows from the room behind the actor's tile alone
        import test_fused_shapes as FS
        room = MS.FB_LDS_LIMIT - FS.fb_lds_bytes(U.SHAPES[case_opts.path]["net"][3], A)
        assert (room >= MS.HEAD_LDS) == (form == "staged"), room
    stored = case["cols"][0].shape[0]
    named = torch.zeros(stored, dtype=torch.bool)
    named[case["idx"]] = True
    named_obs = named.clone()
    named_obs[case["nxt"]] = True
    named_obs[case["pair"]] = True
    ld = hgym.smooth_ld(no)
    shadow = path == "bf16-fused"

    def run(side):
        net, A_, out = side.net, side.A, {}
        GB._fresh(net, opts, case)
        cols = [A_.place(t, skew=4 if i < 2 else 0) for i, t in enumerate(case["cols"])]
        kw = {}
        if shadow:
            sh = lambda x, w: torch.nn.functional.pad(x, (0, w - x.shape[1])).to(BF16)
            kw.update(obs_bf16=A_.place(sh(case["cols"][0], net.shadow_ld(0))), priv_bf16=A_.place(sh(case["cols"][1], net.shadow_ld(1))))
        for i, t in enumerate(cols + list(kw.values())):
            keep = named_obs if i == 0 else named      # (the pre-passes gather the fp32 observation rows of successors and partners)
            t.view(U8).view(stored, -1)[(~keep).to(GB.DEV)] = 0xFF
        idx = A_.place(case["idx"])
        src = A_.place(torch.tensor(case["spec"].act_src, dtype=I32))
        sign = A_.place(torch.tensor(case["spec"].act_sign, dtype=F32))
        target, msums = A_.carve((B, A), F32), A_.zeros(2, F64)
        kw.update(pair_idx=A_.place(case["pair"]), mirror=(src, sign, target, msums))
        tn, ts, rows = A_.carve((B, A), F32), A_.carve((B, A), F32), A_.carve((B, ld), F32)
        sums, hp = A_.zeros(4, F64), A_.zeros(hgym.smooth_mirror_partials(B), F32)      # (a row's last two floats are never written)
        assert hp.numel() == 8 and hp.data_ptr() % 16 == 0
        sm = hgym.make_smooth(MS.LAM_T, MS.LAM_S, next_idx=A_.place(case["nxt"]), next_weight=A_.place(case["weight"]),
                              noise_std=A_.place(torch.from_numpy(case["noise_std"])), seed=S.SEED, target_next=tn.view(-1), target_near=ts.view(-1),
                              rows=rows.view(-1), sums=sums)
        ppo = make_ppo_config(grad_norm_ready=False, aux_coef=0.0, clipped_value_loss=True, mirror_coef=MS.COEF)
        net.ppo_grad_smooth_mirror(ppo, make_batch(*cols, idx, **kw), sm, hp)
        side.verify("hgym_ppo_grad_smooth_mirror")
        out["grads_ext"] = net.grads_ext.clone()
        GB._opt_state(net, out, "opt_state after grad")
        out.update(mirror_target=target, mirror_sums=msums, target_next=tn, target_near=ts, rows=rows, sums=sums, head_partials=hp)
        assert float(msums[1]) == 1.0 and float(sums[3]) == 1.0 and float(sums[0]) > 0.0 and float(sums[1]) > 0.0 and float(msums[0]) > 0.0
        net.ppo_apply(ppo)
        side.verify("hgym_ppo_apply")
        out.update(params=net.params.clone(), adam_m=net.adam_m.clone(), adam_v=net.adam_v.clone())
        GB._opt_state(net, out, "opt_state")
        return out
    GB._pair(run, "mirror + smooth update %s %s B=%d" % (path, form, B), nets=nets)
