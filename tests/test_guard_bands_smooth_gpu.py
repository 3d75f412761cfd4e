"""-m gpu: the three entry points of the smoothness regulariser stay inside the caller's buffers (DESIGN.md sections 25 and 28), on
tests/test_guard_bands_gpu.py's twin runs: once on ordinary tensors, once with every pointer carved from a guard_common.Arena at exactly
the size include/hgym.h states; afterwards the bands are clean and the outputs carry the twin's bits."""
import ctypes as C

import pytest
import torch

import guard_common as G
import smoothness_common as S
import test_guard_bands_gpu as GB
import update_options_common as U
from hgym import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, I64, U8, BF16 = torch.float32, torch.float64, torch.int64, torch.uint8, torch.bfloat16


@pytest.mark.parametrize("T,N,B", [(4, 3, 1), (7, 37, 255), (9, 33, 257)])
def test_smooth_pairs(T, N, B):
    def case(side):
        A, g = side.A, GB._gen(T * N + B)
        dones = A.place((torch.rand(T * N, generator=g) < 0.4).to(U8), skew=1)
        idx = A.place(torch.randperm(T * N, generator=g)[:B].contiguous())
        nxt, w = A.carve(B, I64), A.carve(B, F32)
        L.check(L.lib.hgym_smooth_pairs(B, N, L.i64ptr(idx), L.u8ptr(dones), L.i64ptr(nxt), L.fptr(w), GB._s()), "hgym_smooth_pairs")
        side.verify("the call")
        return dict(next_idx=nxt, next_weight=w)
    GB._pair(case, "hgym_smooth_pairs T=%d N=%d B=%d" % (T, N, B))


@pytest.mark.parametrize("gathered", [False, True], ids=["contiguous", "gathered"])
@pytest.mark.parametrize("M,width", [(1, 5), (63, 47), (130, 705), (65, 8)])
def test_perturb_rows(M, width, gathered):
    """src rows of width + 3 floats whose tails are 0xFF, carved at a 4-byte address; dst exactly (M, width rounded up to 4), 16-byte aligned;
    noise_std exactly `width` floats; rows no index names are 0xFF."""
    ld_src, ld = width + 3, (width + 3) // 4 * 4
    rows = 2 * M + 3 if gathered else M

    def case(side):
        A, g = side.A, GB._gen(1000 * M + width)
        src = A.carve((rows, ld_src), F32, skew=4)
        perm = torch.randperm(rows, generator=g)
        named = perm[:M] if gathered else torch.arange(M)
        src[named.to(DEV), :width] = torch.randn(M, width, generator=g).to(DEV)
        idx = A.place(named.contiguous()) if gathered else None
        ns = A.place(torch.rand(width, generator=g).float(), skew=4)
        opt = A.zeros(L.OPT_STATE, F64)
        opt[L.OPT_STEP] = 9.0
        dst = A.carve((M, ld), F32)
        L.check(L.lib.hgym_perturb_rows(M, width, L.fptr(src), ld_src, L.i64ptr(idx), L.fptr(ns), 77, L.f64ptr(opt), L.fptr(dst), ld, GB._s()),
                "hgym_perturb_rows")
        side.verify("the call")
        assert GB._all_ff(src[:, width:])
        assert bool((dst[:, width:].contiguous().view(torch.int32) == 0).all())
        return dict(dst=dst, opt_state=opt)
    GB._pair(case, "hgym_perturb_rows M=%d width=%d" % (M, width))


GRAD_CASES = [(p, b, "rows") for p in U.PATHS for b in ((1, 33, 49) if p == "f32-layer" else (1, 33, 97))] + [("bf16-fused", b, "shadow") for b in (1, 97)] + \
             [("bf16-fused", 97, "tanh"), ("bf16-fused", 97, "temporal"), ("bf16-fused", 97, "spatial")]


@pytest.mark.parametrize("path,B,variant", GRAD_CASES, ids=["%s-B%d-%s" % c for c in GRAD_CASES])
def test_ppo_grad_smooth(path, B, variant):
    """hgym_ppo_grad_smooth on (T + 1) N stored observation rows of which idx and next_idx name 2 B at most -- every other row of the columns
    and of the shadows is 0xFF.  target_next and target_near are exactly (B, A), rows exactly (B, ld), sums 4 doubles, next_idx and
    next_weight exactly B."""
    from hgym import make_batch, make_ppo_config, make_smooth, smooth_ld
    opts = GB._opts(path, act=U.TANH if variant == "tanh" else None)
    case = S.make_case(opts, seed=300 + B, B=B)
    no, npv, A = GB._dims(opts)
    rows_all = case["cols"][0].shape[0]
    shadow = variant == "shadow"
    lam = (S.LAM_T, 0.0) if variant == "temporal" else (0.0, S.LAM_S) if variant == "spatial" else (S.LAM_T, S.LAM_S)
    unnamed = torch.ones(rows_all, dtype=torch.bool)
    unnamed[case["idx"]] = False
    unnamed_obs = unnamed.clone()
    unnamed_obs[case["nxt"]] = False

    def run(side):
        net, A_, out = side.net, side.A, {}
        GB._fresh(net, opts, case)
        cols = [A_.place(t, skew=4 if i < 2 else 0) for i, t in enumerate(case["cols"])]
        kw = {}
        if shadow:
            sh = lambda x, ld: torch.nn.functional.pad(x, (0, ld - x.shape[1])).to(BF16)
            kw.update(obs_bf16=A_.place(sh(case["cols"][0], net.shadow_ld(0))), priv_bf16=A_.place(sh(case["cols"][1], net.shadow_ld(1))))
        for i, t in enumerate(cols + list(kw.values())):
            t.view(U8).view(rows_all, -1)[(unnamed_obs if i == 0 else unnamed).to(DEV)] = 0xFF      # (the fp32 obs column also serves next_idx)
        idx = A_.place(case["idx"])
        nxt, w = A_.place(case["nxt"]), A_.place(case["weight"])
        ns = A_.place(torch.from_numpy(case["noise_std"]), skew=4)
        tn, ts, pr = A_.carve((B, A), F32), A_.carve((B, A), F32), A_.carve((B, smooth_ld(no)), F32)
        sums = A_.zeros(4, F64)
        net.opt_state[L.OPT_STEP] = 2.0
        ppo = make_ppo_config(grad_norm_ready=False, aux_coef=case["ppo"]["aux_coef"])
        sm = make_smooth(lam[0], lam[1], next_idx=nxt, next_weight=w, noise_std=ns, seed=S.SEED, target_next=tn, target_near=ts, rows=pr, sums=sums)
        net.ppo_grad_smooth(ppo, make_batch(*cols, idx, **kw), sm)
        side.verify("hgym_ppo_grad_smooth")
        out["grads_ext"] = net.grads_ext.clone()
        GB._opt_state(net, out, "opt_state")
        out["sums"] = sums
        if lam[0] > 0:
            out["target_next"] = tn
        else:
            assert GB._all_ff(tn)
        if lam[1] > 0:
            out["target_near"], out["rows"] = ts, pr
        else:
            assert GB._all_ff(ts) and GB._all_ff(pr)
        assert float(sums[3]) == 1.0
        return out
    GB._pair(run, "hgym_ppo_grad_smooth %s B=%d %s" % (path, B, variant), nets=GB._nets(opts))
