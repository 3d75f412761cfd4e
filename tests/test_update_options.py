"""The float64 reference and the cases of the combined update-options matrix (tests/update_options_common.py), pinned
on the host: the reference against the pieces it restates -- oracle/ppo_oracle.py with every option off, the single-option restatements
with one option on -- and the cases against the condition that keeps the GPU test from passing a kernel that ignores a switch."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import fused_batch_common as FB
import loss_head_common as H
import obs_norm_common as ON
import update_options_common as U
from oracle import ppo_oracle as P

IDS = [U.case_id(o) for o in U.MATRIX]


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _opts(path, **kw):
    return U.Options(path, None, "scalar", False, False, False, False)._replace(**kw)


def _oracle_params(case):
    p = case["params"]
    lay = lambda net: U._layers(p, net, torch.float64)
    return P.Params(lay("actor"), lay("critic"), p["std"].double())


# ------------------------------------------------------------------------------------------------ all options off
@pytest.mark.parametrize("quant", [None, "bf16"])
@pytest.mark.parametrize("path", U.PATHS)
def test_all_options_off_is_the_oracle(path, quant):
    """reference == oracle/ppo_oracle.py::ppo_loss_and_grads (hand-written backward, ELU(1), scalar std, clipped loss) in float64, 1e-12
    relative per tensor, on every path's shape, with and without the bf16 operand rounding."""
    case = U.make_case(_opts(path), seed=3)
    q = FB.q64 if quant else None
    got = U.reference(case["opts"], case["params"], None, case["cols"], case["idx"], case["ppo"], quant=q)
    sel = [t[case["idx"]].double() for t in case["cols"]]
    with torch.no_grad():
        want = P.ppo_loss_and_grads(_oracle_params(case), *sel, clip=case["ppo"]["clip"], value_coef=case["ppo"]["value_coef"],
                                    entropy_coef=case["ppo"]["entropy_coef"], quant=q)
    for k, w in zip(U.names_of(case["opts"]), want["grads"].tensors()):
        assert float(w.abs().max()) > 0, k
        assert _rel(got["grads"][k], w) <= 1e-12, (k, _rel(got["grads"][k], w))
    for k, kw in (("surrogate", "surrogate"), ("value", "value_loss"), ("entropy", "entropy"), ("kl", "kl")):
        assert _rel(got["sums"][k], want[kw]) <= 1e-12, k
    assert _rel(got["d_val"], want["d_val"]) <= 1e-12 and _rel(got["d_mu"], want["d_mu"]) <= 1e-12


# ------------------------------------------------------------------------------------------------ one option on
@pytest.mark.parametrize("unclipped", [False, True])
@pytest.mark.parametrize("path", U.PATHS)
def test_head_against_the_loss_head_restatement(path, unclipped):
    """The head's sums and its d_mu, d_val, d_std against tests/loss_head_common.py::reference (per-sample float64 autograd), clipped and
    unclipped, 1e-10."""
    case = U.make_case(_opts(path, unclipped=unclipped), seed=4)
    o = case["opts"]
    ref = U.reference(o, case["params"], None, case["cols"], case["idx"], case["ppo"])
    sel = [t[case["idx"]] for t in case["cols"]]
    mu, v, _ = U.forward(o, case["params"], None, sel[0], sel[1])
    rows = dict(zip(("actions", "values", "adv", "returns", "logp", "mu_old", "sigma_old"), sel[2:]))
    want = H.reference(rows, mu, v, case["params"]["std"], ppo=case["ppo"], unclipped=unclipped)
    for k, kw in (("surrogate", "surr"), ("value", "vl"), ("entropy", "ent"), ("kl", "kl")):
        assert _rel(ref["sums"][k], want[kw].mean()) <= 1e-10, k
    assert _rel(ref["d_mu"], want["g_mu"]) <= 1e-10 and _rel(ref["d_val"], want["d_v"]) <= 1e-10
    assert _rel(ref["grads"]["std"], want["g_sigma"].sum(0)) <= 1e-10
    # the two forms differ on this case: about half the rows are dropped by the clipped one
    other = U.reference(o._replace(unclipped=not unclipped), case["params"], None, case["cols"], case["idx"], case["ppo"])
    assert _rel(other["d_val"], ref["d_val"]) > 0.1


@pytest.mark.parametrize("path", U.PATHS)
def test_log_std_gradient_is_the_scalar_one_times_sigma(path):
    case = U.make_case(_opts(path, std="log"), seed=5)
    o = case["opts"]
    ref = U.reference(o, case["params"], None, case["cols"], case["idx"], case["ppo"])
    so, sp = U.flipped(case, "std")
    assert list(sp)[0] == "std" and so.std == "scalar"
    sigma = U.sigma_of(o, case["params"])
    assert _rel(sigma, sp["std"]) <= 1e-6
    sp["std"] = sigma       # (flipped() rounds it to fp32, for a device to load; here the same sigma to the last float64 bit)
    scal = U.reference(so, sp, None, case["cols"], case["idx"], case["ppo"])
    assert float((sigma - 1).abs().min()) >= 0.39
    assert _rel(ref["grads"]["log_std"], scal["grads"]["std"] * sigma) <= 1e-10
    for k in U.names_of(o)[1:]:
        assert _rel(ref["grads"][k], scal["grads"][k]) <= 1e-10, k
    for k in ("surrogate", "value", "entropy", "kl"):
        assert _rel(ref["sums"][k], scal["sums"][k]) <= 1e-10, k


@pytest.mark.parametrize("aux", [False, True])
def test_normalised_f32_case_is_plain_autograd_on_normalised_rows(aux):
    """norm on, f32: the folded / unfolded reference == float64 autograd of the loss on obs_norm_common.normalise'd rows in the MASTER
    parametrisation -- no fold, no unfold (the auxiliary targets stay raw columns of the privileged row), 1e-10."""
    case = U.make_case(_opts("f32-layer", norm=True, aux=aux), seed=6)
    o, ppo = case["opts"], case["ppo"]
    ref = U.reference(o, case["params"], case["stats"], case["cols"], case["idx"], ppo)
    (m0, s0), (m1, s1) = U.derived_stats(case["stats"])
    assert np.abs(m0 * s0).max() > 2.9 and (np.asarray(case["stats"]["var"][0]) == 0).sum() == 1
    sel = [t[case["idx"]].double() for t in case["cols"]]
    raw_priv = sel[1]
    sel[0] = torch.from_numpy(ON.normalise(sel[0].numpy(), m0, s0))
    sel[1] = torch.from_numpy(ON.normalise(sel[1].numpy(), m1, s1))
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in case["params"].items()}
    lay = lambda net: U._layers(leaves, net, torch.float64)
    loss = P.ppo_loss_and_grads(P.Params(lay("actor"), lay("critic"), leaves["std"]), *sel, clip=ppo["clip"], value_coef=ppo["value_coef"],
                                entropy_coef=ppo["entropy_coef"])["loss"]
    if aux:
        _, out, off = U.SHAPES["f32-layer"]["aux"]
        assert off == raw_priv.shape[1] - out
        y = P.mlp_forward(sel[0], lay("denoiser"))
        loss = loss + ppo["aux_coef"] * ((y - raw_priv[:, off:off + out]) ** 2).mean()
    loss.backward()
    for k in U.names_of(o):
        assert _rel(ref["grads"][k], leaves[k].grad) <= 1e-10, (k, _rel(ref["grads"][k], leaves[k].grad))
    # ... and it is not the gradient of the same net on the raw rows
    raw = U.reference(o._replace(norm=False), case["params"], None, case["cols"], case["idx"], ppo)
    assert _rel(raw["grads"]["actor.0.weight"], ref["grads"]["actor.0.weight"]) > 0.1


@pytest.mark.parametrize("path", ["f32-layer", "bf16-layer"])
def test_auxiliary_gradient_is_autograd_of_a_sequential_twin(path):
    case = U.make_case(_opts(path, aux=True), seed=7)
    o, ppo = case["opts"], case["ppo"]
    ref = U.reference(o, case["params"], None, case["cols"], case["idx"], ppo, quant=None)
    hidden, out, off = U.SHAPES[path]["aux"]
    assert off == U.SHAPES[path]["net"][1] - out
    dims = [U.SHAPES[path]["net"][0]] + hidden + [out]
    mods = []
    for l in range(len(dims) - 1):
        lin = nn.Linear(dims[l], dims[l + 1]).double()
        with torch.no_grad():
            lin.weight.copy_(case["params"]["denoiser.%d.weight" % (2 * l)])
            lin.bias.copy_(case["params"]["denoiser.%d.bias" % (2 * l)])
        mods += [lin] + ([nn.ELU()] if l < len(dims) - 2 else [])
    twin = nn.Sequential(*mods)
    x, xp = (case["cols"][k][case["idx"]].double() for k in (0, 1))
    mse = ((twin(x) - xp[:, off:off + out]) ** 2).mean()
    (ppo["aux_coef"] * mse).backward()
    assert _rel(ref["sums"]["aux"], mse.detach()) <= 1e-10
    for l, lin in enumerate(m for m in twin if isinstance(m, nn.Linear)):
        assert _rel(ref["grads"]["denoiser.%d.weight" % (2 * l)], lin.weight.grad) <= 1e-10, l
        assert _rel(ref["grads"]["denoiser.%d.bias" % (2 * l)], lin.bias.grad) <= 1e-10, l
    # the head leaves the PPO part alone
    plain = U.reference(*U.flipped(case, "aux"), None, case["cols"], case["idx"], U.ppo_constants(o._replace(aux=False)), quant=None)
    for k, g in plain["grads"].items():
        assert torch.equal(g, ref["grads"][k]), k


def test_fp32_evaluation_of_the_reference_is_close_to_float64():
    """reference(dtype=float32) -- what test a of the GPU file falls back on to tell fp32 accumulation from a wrong kernel -- runs every
    option and lands within the fp32 bar of the float64 result on the f32 path."""
    o = U.Options("f32-layer", U.TANH, "log", True, True, True, False)
    case = U.case_of(o)
    r64, r32 = U.reference_of(o), U.reference(o, case["params"], case["stats"], case["cols"], case["idx"], case["ppo"], dtype=torch.float32)
    errs = U.errors(o, r32["grads"], r64)
    assert all(r32["grads"][k].dtype == torch.float32 for k in errs) and max(errs.values()) <= U.F32_GRAD_TOL, errs


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("opts", U.MATRIX, ids=IDS)
def test_every_option_matters_in_every_case(opts):
    """For every case and every option but `shadow`: the reference with that ONE option flipped moves at least one tensor's gradient by
    more than 10 x the bar the GPU test applies to that tensor, in the GPU test's own metric (update_options_common.errors).  The
    auxiliary head is judged on the denoiser.* tensors, present against absent: present, each of them against zero; absent, the twin
    case with the head is in the matrix and is judged there.  Also: the case is what make_case promises -- about a third of the ratios
    outside 1 +- clip and none near a bound, about half the rows with the old value beyond the clip range on the returns' far side."""
    case, ref = U.case_of(opts), U.reference_of(opts)
    o = case["opts"]
    bar = U.bar_of(o)
    for k, g in ref["grads"].items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
    for option in U.FLIPPABLE:
        if option == "aux":
            if not o.aux:
                assert o._replace(aux=True, shadow=opts.shadow) in U.MATRIX
                continue
            den = [k for k in ref["grads"] if k.startswith("denoiser.")]
            assert len(den) == 2 * (len(U.SHAPES[o.path]["aux"][0]) + 1)
            moved = U.errors(o, {k: torch.zeros_like(ref["grads"][k]) for k in den}, ref, names=den)
        else:
            fo, fp = U.flipped(case, option)
            other = U.reference(fo, fp, case["stats"], case["cols"], case["idx"], case["ppo"])
            got = dict(zip(ref["grads"], other["grads"].values()))      # (std <-> log_std: the same slot under another name)
            moved = U.errors(o, got, ref)
        assert max(moved.values()) > U.SENSITIVITY * bar, (option, max(moved.values()), bar)
    # the case itself
    sel = [t[case["idx"]] for t in case["cols"]]
    mu, v, _ = U.forward(o, case["params"], case["stats"], sel[0], sel[1])
    sigma = U.sigma_of(o, case["params"])
    log_ratio = P.gaussian_log_prob(sel[2].double(), mu, mu * 0 + sigma) - sel[6].double()
    outside = (log_ratio > np.log1p(0.2)) | (log_ratio < np.log1p(-0.2))
    assert 0.15 <= float(outside.double().mean()) <= 0.55
    assert float(torch.minimum((log_ratio - np.log1p(0.2)).abs(), (log_ratio - np.log1p(-0.2)).abs()).min()) > 0.05
    d = v - sel[3].double()
    far = (d.abs() > 0.2) & (torch.sign(d) == torch.sign(sel[5].double() - v))       # V between the old value and the returns
    assert 0.3 <= float(far.double().mean()) <= 0.7 and float((d.abs() - 0.2).abs().min()) > 0.05
    assert float((sigma - 1).abs().min()) >= 0.39 and bool((case["idx"] != torch.arange(case["B"])).any()) and case["S"] > case["B"]


def test_matrix():
    assert len(U.MATRIX) == 128 and len(set(U.MATRIX)) == 128 and len(set(IDS)) == 128
    count = lambda path: sum(1 for o in U.MATRIX if o.path == path)
    assert (count("bf16-fused"), count("f32-layer"), count("bf16-layer")) == (64, 32, 32)
    assert all(not o.shadow for o in U.MATRIX if o.path != "bf16-fused")
    for path in U.PATHS:      # the full factorial
        seen = {(o.activation is not None, o.std, o.unclipped, o.aux, o.norm, o.shadow) for o in U.MATRIX if o.path == path}
        assert len(seen) == count(path)
    sh = U.SHAPES["bf16-fused"]
    pl = FB.plan(sh["B"])
    assert pl["tiles"] == 2 and sh["B"] - 64 == 33 and pl["tail_rows"] == 1      # two update tiles, the second ragged, one row in its last step


def test_design_section_names_the_files_that_exist():
    """DESIGN.md section 23 and README.md name this file, its GPU twin and the common module by file name; they are here."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    docs = {d: open(os.path.join(os.path.dirname(here), d)).read() for d in ("DESIGN.md", "README.md")}
    for name in ("test_update_options.py", "test_update_options_gpu.py", "update_options_common.py"):
        assert os.path.exists(os.path.join(here, name)) and name in docs["DESIGN.md"], name
    assert "test_update_options_gpu.py" in docs["README.md"] and "## 23. " in docs["DESIGN.md"]


# ------------------------------------------------------------------------------------------------ mirror_columns
def test_mirror_columns_is_an_involution_that_moves_every_mirrored_column():
    spec = U.xbot_l_spec()
    g = torch.Generator().manual_seed(9)
    M = 7
    cols = [torch.randn(M, w, generator=g) for w in (705, 219, 12)] + [torch.randn(M, generator=g) for _ in range(4)] + \
           [torch.randn(M, 12, generator=g), torch.rand(M, 12, generator=g) + 0.5]
    once = U.mirror_columns(cols, spec)
    assert all(t.shape[0] == 2 * M for t in once)
    for a, b in zip(cols, once):
        assert torch.equal(a, b[:M])
    twice = U.mirror_columns([t[M:] for t in once], spec)
    bits = lambda t: t.contiguous().view(torch.int32)
    for k, (a, b) in enumerate(zip(cols, twice)):
        assert torch.equal(bits(a), bits(b[M:])), k
    for k in (0, 1, 2, 7, 8):       # obs, priv, actions, mu, sigma: at least one column moved
        assert bool((once[k][M:] != cols[k]).any(dim=0).any()), k
    for k in (3, 4, 5, 6):          # the scalar columns: repeated
        assert torch.equal(once[k][M:], cols[k])
    assert bool((once[8][M:] > 0).all())       # sigma keeps its sign
    # the tables' own reading: out[c] = sign[c] * in[src[c]]
    c = 5
    assert torch.equal(once[0][M:, c], spec.obs_sign[c] * cols[0][:, spec.obs_src[c]])
