"""Shared by tests/test_update_options.py (CPU) and tests/test_update_options_gpu.py (-m gpu): the PPO update with its options COMBINED
 -- activation, noise parametrisation, value loss, auxiliary head, observation normalisation, bf16 input shadows,
symmetry -- against ONE float64 reference.

  Options       one combination: path ("f32-layer", "bf16-layer", "bf16-fused"), activation (None = ELU(1), or TANH), std ("scalar",
                "log"), unclipped, aux, norm, shadow (fused path only).
  reference     the gradient of the MASTER parameters, keyed by state-dict names, and the minibatch's loss sums.  Built from pieces the
                suite already holds: the bodies are layer_path_common.restated (quant = bf16 rounding on the bf16 paths); the head is
                written once in float64 torch and differentiated by autograd ON THE HEAD ALONE (d_mu, d_val, d_y_aux, d_std); under
                normalisation the bodies are fed the folded first layers (obs_norm_common.fold / operand) and the first-layer weight
                gradients are unfolded (obs_norm_common.unfold).  On the f32 path the fold is evaluated in float64 -- there the reference
                is exactly the master net on normalised rows, and the kernels' one fp32 rounding of w s is part of what the 5e-5 bar covers.
  make_case     stored columns, index slice, parameters and planted statistics built so that every option matters.
  errors        the metric and the bars the GPU test applies per tensor; tests/test_update_options.py holds the reference to them too
                (sensitivity: flipping one option moves some tensor by more than SENSITIVITY x its bar).
  mirror_columns  [rows | mirrored rows] in plain torch indexing from humanoid.utils.symmetry's tables.
  _alg, _fill_rollout, _record_batches   the update harness of tests/test_symmetry_gpu.py (moved here unchanged)."""
import collections
import functools
import itertools

import numpy as np
import torch
import torch.nn as nn

import fused_batch_common as FB
import layer_path_common as LP
import loss_head_common as H
import obs_norm_common as ON
from oracle import ppo_oracle as P

DEV = "cuda"
TANH = nn.Tanh()      # ONE module object: Options compare and hash by it
Options = collections.namedtuple("Options", "path activation std unclipped aux norm shadow")
PATHS = ("bf16-fused", "f32-layer", "bf16-layer")
FLIPPABLE = ("activation", "std", "unclipped", "aux", "norm")      # every option but `shadow`, which must change no bit

# path: net shape, auxiliary head (hidden, outputs, target offset), stored rows S > minibatch B
SHAPES = {
    # XBot-L's widths; two update tiles, the second ragged with 33 rows, its last 32-row step holding one row
    "bf16-fused": dict(net=(705, 219, 12, [512, 256, 128], [768, 256, 128]), aux=([512, 256, 128], 73, 219 - 73), S=130, B=97),
    # the ragged shape the suite uses for this path (tests/test_obs_norm_gpu.py)
    "f32-layer": dict(net=(37, 19, 5, [24, 16], [24, 16]), aux=([24, 16], 7, 19 - 7), S=50, B=33),
    # widths the fused tiles refuse (tests/test_fused_activations_gpu.py SHAPES["big_actor"]), tests/test_aux_head_gpu.py's generic head
    "bf16-layer": dict(net=(705, 219, 12, [768, 256, 128], [768, 256, 128]), aux=([256, 128, 64], 73, 146), S=130, B=97),
}
AUX_COEF = 0.5
EPS = 1e-2            # the normaliser's eps of every case
PLANTED_COUNT = 1000.0

BF16_OPERAND_TOL = FB.BF16_OPERAND_TOL      # 5e-3, rel-L2 per tensor, both bf16 paths
F32_GRAD_TOL = 5e-5                          # max-abs error over max-abs reference (tests/test_layer_path_shapes_gpu.py, tests/test_obs_norm_gpu.py)
SENSITIVITY = 10.0
# the loss sums (opt_state's named slots), relative: tests/test_value_loss_gpu.py holds the fp32 value loss to 1e-5, tests/test_fused_activations_gpu.py
# and tests/test_aux_head_gpu.py the bf16 value loss and auxiliary MSE to 1e-2 (rtol).  The surrogate and the entropy are means of signed
# terms: they are held against the mean of the terms' absolute values (the size of what is summed), like the last critic bias below.
SUM_TOL = {"f32-layer": 1e-5, "bf16-layer": 1e-2, "bf16-fused": 1e-2}


def matrix():
    out = []
    for path in PATHS:
        shadows = (False, True) if path == "bf16-fused" else (False,)
        for act, std, unclipped, aux, norm, shadow in itertools.product((None, TANH), ("scalar", "log"), (False, True), (False, True),
                                                                        (False, True), shadows):
            out.append(Options(path, act, std, unclipped, aux, norm, shadow))
    return out


MATRIX = matrix()


def case_id(o):
    parts = [o.path, "tanh" if o.activation is not None else "elu", o.std, "vu" if o.unclipped else "vc", "aux" if o.aux else "noaux",
             "norm" if o.norm else "raw"]
    if o.path == "bf16-fused":
        parts.append("shadow" if o.shadow else "fp32rows")
    return "-".join(parts)


def quant_of(opts):
    return None if opts.path == "f32-layer" else FB.q64


def ppo_constants(opts):
    """The coefficients as the C struct carries them (fp32-rounded), plus the auxiliary head's."""
    return dict(H.ppo_constants(), aux_coef=H.f32(AUX_COEF) if opts.aux else 0.0)


def names_of(opts):
    """State-dict names of the case's net, in the flat vector's order."""
    _, _, _, ah, ch = SHAPES[opts.path]["net"]
    out = ["log_std" if opts.std == "log" else "std"]
    nets = [("actor", len(ah) + 1), ("critic", len(ch) + 1)]
    if opts.aux:
        nets.append(("denoiser", len(SHAPES[opts.path]["aux"][0]) + 1))
    return out + ["%s.%d.%s" % (n, 2 * l, k) for n, L_ in nets for l in range(L_) for k in ("weight", "bias")]


def last_critic_bias(names):
    return "critic.%d.bias" % max(int(k.split(".")[1]) for k in names if k.startswith("critic."))


# ------------------------------------------------------------------------------------------------ the reference
def _layers(params, net, dtype):
    out, l = [], 0
    while "%s.%d.weight" % (net, 2 * l) in params:
        out.append((params["%s.%d.weight" % (net, 2 * l)].to(dtype), params["%s.%d.bias" % (net, 2 * l)].to(dtype)))
        l += 1
    return out


def derived_stats(stats):
    """[(m, s) of the actor's rows, (m, s) of the critic's]: the kernels' floats (obs_norm_common.derived)."""
    return [ON.derived(stats["mean"][k], stats["var"][k], stats["eps"]) for k in (0, 1)]


def folded(layers, m, s, opts, dtype=torch.float64):
    """The net that takes RAW rows: first layer (Wop, b').  bf16 paths: Wop = the fp32 product w s (the body rounds it to bf16 as the
    operand copy is) and b' = b - T(w s) m from the operand AS ROUNDED; f32: both in float64 (module docstring)."""
    W, b = layers[0]
    if opts.path == "f32-layer":
        Wop = W.double() * torch.from_numpy(np.asarray(s, np.float64))[None, :]
        bp = b.double() - (Wop * torch.from_numpy(np.asarray(m, np.float64))[None, :]).sum(dim=1)
    else:
        _, bp, _ = ON.fold(W.float().numpy(), b.float().numpy(), m, s, "bf16")
        Wop, bp = torch.from_numpy(ON.operand(W.float().numpy(), s, "f32")), torch.from_numpy(bp)
    return [(Wop.to(dtype), bp.to(dtype))] + list(layers[1:])


def bodies(opts, params, stats, dtype=torch.float64):
    """{net: layers as the kernels' products see them (folded under normalisation)} and the (m, s) pairs (None without normalisation)."""
    nets = {n: _layers(params, n, dtype) for n in ("actor", "critic", "denoiser")}
    if not opts.aux:
        nets["denoiser"] = []
    ms = None
    if opts.norm:
        ms = derived_stats(stats)
        nets["actor"] = folded(nets["actor"], *ms[0], opts, dtype)
        nets["critic"] = folded(nets["critic"], *ms[1], opts, dtype)
        if opts.aux:
            nets["denoiser"] = folded(nets["denoiser"], *ms[0], opts, dtype)      # the head reads the actor's rows: the actor's statistics
    return nets, ms


def sigma_of(opts, params, dtype=torch.float64):
    p = params["log_std" if opts.std == "log" else "std"].to(dtype)
    return torch.exp(p) if opts.std == "log" else p


def forward(opts, params, stats, obs, priv, dtype=torch.float64):
    """(mu, V, auxiliary output or None) of raw rows under the options."""
    fwd, _ = LP.restated(opts.activation)
    nets, _ = bodies(opts, params, stats, dtype)
    q = quant_of(opts)
    with torch.no_grad():
        mu = fwd(obs.to(dtype), nets["actor"], quant=q)
        v = fwd(priv.to(dtype), nets["critic"], quant=q).squeeze(-1)
        y = fwd(obs.to(dtype), nets["denoiser"], quant=q) if opts.aux else None
    return mu, v, y


def head(opts, rows, mu, v, y_aux, target, p_std, ppo):
    """The loss head once, in torch: the PPO surrogate, entropy and KL (ppo.py:128-168), the clipped value loss or (R - V)^2, sigma = p or
    exp(p), the auxiliary head's aux_coef * mean_b sum_j (y - t)^2 / aux_out.  autograd ON THE HEAD ALONE: -> dict(d_mu, d_val, d_y_aux,
    d_std (with respect to the PARAMETER), and the minibatch means surrogate, value, entropy, kl, aux, surrogate_abs)."""
    act, vold, adv, ret, lpo, mo, so = rows
    B, A = act.shape
    clip, vcoef, ecoef = ppo["clip"], ppo["value_coef"], ppo["entropy_coef"]
    mu = mu.detach().clone().requires_grad_()
    v = v.detach().clone().requires_grad_()
    p = p_std.detach().clone().requires_grad_()
    sig = (torch.exp(p) if opts.std == "log" else p).expand(B, A)
    logp = P.gaussian_log_prob(act, mu, sig)
    ent = P.gaussian_entropy(sig)
    kl = torch.sum(torch.log(sig / so + 1.e-5) + (so ** 2 + (mo - mu) ** 2) / (2.0 * sig ** 2) - 0.5, dim=-1)
    ratio = torch.exp(logp - lpo)
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if opts.unclipped:
        vl = (ret - v).pow(2)
    else:
        vc = vold + (v - vold).clamp(-clip, clip)
        vl = torch.max((v - ret).pow(2), (vc - ret).pow(2))
    loss = surr.mean() + vcoef * vl.mean() - ecoef * ent.mean()
    leaves = [mu, v, p]
    aux = None
    if opts.aux:
        y = y_aux.detach().clone().requires_grad_()
        aux = ((y - target) ** 2).sum(dim=-1).mean() / y.shape[1]
        loss = loss + ppo["aux_coef"] * aux
        leaves.append(y)
    g = torch.autograd.grad(loss, leaves)
    return dict(d_mu=g[0], d_val=g[1], d_std=g[2], d_y_aux=g[3] if opts.aux else None, surrogate=surr.mean().detach(),
                value=vl.mean().detach(), entropy=ent.mean().detach(), kl=kl.mean().detach(), aux=None if aux is None else aux.detach(),
                surrogate_abs=surr.abs().mean().detach(), entropy_abs=(0.5 + P.HALF_LOG_2PI + torch.log(sig).abs()).sum(-1).mean().detach())


AUTO = object()


def reference(opts, params, stats, cols, idx, ppo, dtype=torch.float64, quant=AUTO):
    """-> dict(grads: {state-dict name: gradient of the master parameter}, sums: {surrogate, value, entropy, kl, aux, surrogate_abs},
    d_val, d_mu).  params: {state-dict name: tensor}; stats: dict(mean=[obs, priv], var=[...], eps) (read under opts.norm only); cols:
    the nine stored columns (obs, priv, actions, values, advantages, returns, logp, mu, sigma); idx: the minibatch's rows.
    dtype: float64; float32 evaluates the same code in fp32 (what fp32 accumulation alone costs a combination).  quant: the bodies'
    operand rounding, by default the path's (bf16 rounding on the bf16 paths, none on f32)."""
    fwd, bwd = LP.restated(opts.activation)
    q = quant_of(opts) if quant is AUTO else quant
    nets, ms = bodies(opts, params, stats, dtype)
    sel = [t[idx].to(dtype) for t in cols]
    X, XP = sel[0], sel[1]
    with torch.no_grad():
        mu, a_acts, a_pres = fwd(X, nets["actor"], keep=True, quant=q)
        v, c_acts, c_pres = fwd(XP, nets["critic"], keep=True, quant=q)
        y = target = None
        if opts.aux:
            y, x_acts, x_pres = fwd(X, nets["denoiser"], keep=True, quant=q)
            target = XP[:, XP.shape[1] - y.shape[1]:]      # the privileged row's LAST aux_out columns (every case's aux_target_offset): raw, never rounded, never normalised
    p_name = "log_std" if opts.std == "log" else "std"
    hd = head(opts, sel[2:], mu, v.squeeze(-1), y, target, params[p_name].to(dtype), ppo)
    with torch.no_grad():
        got = {"actor": bwd(hd["d_mu"], nets["actor"], a_acts, a_pres, quant=q),
               "critic": bwd(hd["d_val"].unsqueeze(1), nets["critic"], c_acts, c_pres, quant=q)}
        if opts.aux:
            got["denoiser"] = bwd(hd["d_y_aux"], nets["denoiser"], x_acts, x_pres, quant=q)
    grads = {p_name: hd["d_std"]}
    for net, g in got.items():
        for l, (gW, gb) in enumerate(g):
            if l == 0 and opts.norm:
                m, s = ms[1] if net == "critic" else ms[0]
                gW = torch.from_numpy(ON.unfold(gW.double().numpy(), gb.double().numpy(), m, s)).to(dtype)
            grads["%s.%d.weight" % (net, 2 * l)], grads["%s.%d.bias" % (net, 2 * l)] = gW, gb
    assert list(grads) == [k for k in params if opts.aux or not k.startswith("denoiser.")]
    sums = {k: hd[k] for k in ("surrogate", "value", "entropy", "kl", "aux", "surrogate_abs", "entropy_abs")}
    return dict(grads=grads, sums=sums, d_val=hd["d_val"], d_mu=hd["d_mu"])


# ------------------------------------------------------------------------------------------------ the metric and the bars
def bar_of(opts):
    return F32_GRAD_TOL if opts.path == "f32-layer" else BF16_OPERAND_TOL


def errors(opts, got, ref, names=None):
    """{tensor: error of got[tensor] against ref["grads"][tensor] in the GPU test's metric}: rel-L2 on the bf16 paths, max-abs error over
    max-abs reference on f32; the critic's last bias -- ONE number, the sum of the per-sample d_val, which cancel -- against ||d_val||
    (tests/test_activations_gpu.py)."""
    out, last = {}, last_critic_bias(ref["grads"])
    for k in names or ref["grads"]:
        a, r = torch.as_tensor(got[k]).double().flatten(), ref["grads"][k].double().flatten()
        if k == last:
            out[k] = float((a - r).norm() / ref["d_val"].double().norm())
        elif opts.path == "f32-layer":
            out[k] = float((a - r).abs().max() / r.abs().max().clamp_min(1e-300))
        else:
            out[k] = FB.rel_l2(a, r)
    return out


def sum_errors(opts, got, ref):
    """{loss sum: relative error}; got: {surrogate, value, entropy, kl, aux} as read from opt_state's named slots."""
    s = ref["sums"]
    out = {k: abs(float(got[k]) - float(s[k])) / abs(float(s[k])) for k in ("value", "kl")}      # sums of non-negative terms
    out["entropy"] = abs(float(got["entropy"]) - float(s["entropy"])) / float(s["entropy_abs"])
    out["surrogate"] = abs(float(got["surrogate"]) - float(s["surrogate"])) / float(s["surrogate_abs"])
    if opts.aux:
        out["aux"] = abs(float(got["aux"]) - float(s["aux"])) / abs(float(s["aux"]))
    return out


# ------------------------------------------------------------------------------------------------ cases
def make_stats(K, g):
    """Planted statistics of K = (num_obs, num_priv) columns as tests/test_obs_norm_gpu.py::_planted_general makes them: |m| s <= 3, one
    var = 0 column per kind, eps = 1e-2."""
    from test_obs_norm_gpu import _planted_general
    means, variances = _planted_general(K, EPS, g)
    return dict(mean=means, var=variances, eps=EPS)


def unit_row_stats(K, g):
    """Statistics under which N(0, 1) rows stay O(1) -- for rollouts whose rows are drawn, not made for the statistics: means in
    [-0.5, 0.5], variances in [0.5, 2]; far enough from the identity (mean 0, var 1) that ignoring them is seen."""
    r = lambda k: torch.rand(k, generator=g, dtype=torch.float64).numpy()
    return dict(mean=[r(k) - 0.5 for k in K], var=[0.5 * 4.0 ** r(k) for k in K], eps=EPS)


def norm_state_of(stats, count=PLANTED_COUNT):
    """NetBuffers.load_norm_state's argument."""
    t = torch.from_numpy
    return dict(obs=dict(mean=t(stats["mean"][0]), var=t(stats["var"][0]), count=count),
                critic_obs=dict(mean=t(stats["mean"][1]), var=t(stats["var"][1]), count=count))


def make_params(opts, g):
    """{state-dict name: fp32 tensor}: nn.Linear's default init (oracle/ppo_oracle.py Params.random); sigma from [0.3, 0.6] U [1.5, 2.5]
    (far from 1: the log and the scalar parametrisation's gradients differ by the factor sigma), stored as itself or as its logarithm."""
    no, npv, A, ah, ch = SHAPES[opts.path]["net"]
    p = P.Params.random(no, npv, A, ah, ch, g)
    u = torch.rand(A, generator=g)
    sigma = torch.where(torch.arange(A) % 2 == 0, 0.3 + 0.3 * u, 1.5 + u)[torch.randperm(A, generator=g)]
    xh, xo, _ = SHAPES[opts.path]["aux"]
    den = P.Params.random(no, 8, xo, xh, [8], g).actor      # drawn whether the case has the head or not: the same numbers either way
    tensors = [torch.log(sigma) if opts.std == "log" else sigma] + p.tensors()[1:]
    if opts.aux:
        tensors += [t for wb in den for t in wb]
    return dict(zip(names_of(opts), [t.float().contiguous() for t in tensors]))


def make_case(opts, S=None, B=None, seed=0):
    """-> dict(opts, params, stats, cols (nine fp32 columns of S rows), idx (B of the S rows, a slice of a permutation), ppo, S, B).
    Every option matters:
      * the rows: raw rows drawn around the planted means under normalisation (m + (sqrt(var) + eps) z), N(0, 1) rows otherwise;
      * actions mu + sigma z, |z| <= 2; old log-probabilities the current policy's (the float64 reference forward under the case's own
        options) plus a log ratio that lies within +-0.1 on two thirds of the rows and at +-[0.4, 0.8] on one third: about a third of
        the ratios outside 1 +- clip, none near a bound (log 1.2 = 0.18, log 0.8 = -0.22);
      * old values: on about half the rows 0.5 > clip away from V ON THE RETURNS' FAR SIDE (V lies between them, the clipped value is
        further from the returns than V and the clipped form drops the row, the unclipped one keeps it), else within +-0.1 of V."""
    sh = SHAPES[opts.path]
    S, B = S or sh["S"], B or sh["B"]
    assert S > B
    no, npv, A = sh["net"][:3]
    g = torch.Generator().manual_seed(1000 + seed)
    stats = make_stats((no, npv), g)
    params = make_params(opts, g)
    if opts.norm:
        from test_obs_norm_gpu import _raw_rows
        e32 = float(np.float32(EPS))
        obs, priv = (torch.from_numpy(_raw_rows(S, stats["mean"][k], stats["var"][k], e32, g)) for k in (0, 1))
    else:
        obs, priv = torch.randn(S, no, generator=g), torch.randn(S, npv, generator=g)
    mu, v, _ = forward(opts, params, stats, obs, priv)
    sigma = sigma_of(opts, params)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    sign = lambda *s: torch.where(r(*s) < 0.5, -1.0, 1.0).double()
    act = mu + sigma * torch.randn(S, A, generator=g, dtype=torch.float64).clamp(-2.0, 2.0)
    out = torch.arange(S) % 3 == 0      # by row number, not by chance: a small minibatch holds its share of either kind
    log_ratio = torch.where(out, sign(S) * (0.4 + 0.4 * r(S)), 0.2 * r(S) - 0.1)
    lp_o = P.gaussian_log_prob(act.float().double(), mu, mu * 0 + sigma) - log_ratio
    ret = v + sign(S) * (0.3 + r(S))
    far = torch.arange(S) % 2 == 0
    val = torch.where(far, v + torch.sign(v - ret) * 0.5, v + 0.2 * r(S) - 0.1)
    adv = torch.randn(S, generator=g, dtype=torch.float64)
    mu_o = mu + 0.3 * sigma * torch.randn(S, A, generator=g, dtype=torch.float64)
    sg_o = sigma * (0.8 + 0.45 * r(S, A))
    cols = [obs, priv] + [t.float().contiguous() for t in (act, val, adv, ret, lp_o, mu_o, sg_o)]
    idx = torch.randperm(S, generator=g)[:B].contiguous()
    return dict(opts=opts, params=params, stats=stats, cols=cols, idx=idx, ppo=ppo_constants(opts), S=S, B=B)


@functools.lru_cache(maxsize=None)
def case_of(opts):
    """make_case of a MATRIX entry at its path's shape.  `shadow` does not enter: the two variants of a fused case share inputs."""
    o = opts._replace(shadow=False)
    return make_case(o, seed=MATRIX.index(o))


def reference_of(opts):
    return _reference_of(opts._replace(shadow=False))


@functools.lru_cache(maxsize=None)
def _reference_of(opts):
    c = case_of(opts)
    return reference(c["opts"], c["params"], c["stats"], c["cols"], c["idx"], c["ppo"])


def flipped(case, option):
    """(options, parameters) of the case with ONE option the other way, everything else -- inputs, weights, sigma -- the same.  std: the
    same sigma under the other parametrisation (the head parameter becomes its logarithm / its exponential, under the other name).  aux
    on -> off drops the head's tensors; off -> on is not formed here (the twin case with the head is in MATRIX)."""
    o, params = case["opts"], dict(case["params"])
    if option == "activation":
        return o._replace(activation=TANH if o.activation is None else None), params
    if option == "std":
        n = o._replace(std="scalar" if o.std == "log" else "log")
        items = list(params.items())
        items[0] = ("std", torch.exp(items[0][1].double()).float()) if o.std == "log" else ("log_std", torch.log(items[0][1].double()).float())
        return n, dict(items)
    if option == "aux":
        assert o.aux
        return o._replace(aux=False), {k: v for k, v in params.items() if not k.startswith("denoiser.")}
    return o._replace(**{option: not getattr(o, option)}), params


# ------------------------------------------------------------------------------------------------ symmetry
def mirror_columns(cols, spec):
    """The nine columns doubled, [rows | mirrored rows]: out[:, c] = sign[c] * in[:, src[c]] for observations, privileged observations,
    actions and mu (the action table), sigma permuted with sign +1, the scalar columns repeated.  Plain torch indexing from the
    MirrorSpec's tables (humanoid/utils/symmetry.py)."""
    def m(x, src, sign):
        return x[:, torch.tensor(src, dtype=torch.int64, device=x.device)] * torch.tensor(sign, dtype=x.dtype, device=x.device)
    obs, priv, act, val, adv, ret, lp, mu, sg = cols
    mirrored = [m(obs, spec.obs_src, spec.obs_sign), m(priv, spec.priv_src, spec.priv_sign), m(act, spec.act_src, spec.act_sign), val, adv,
                ret, lp, m(mu, spec.act_src, spec.act_sign), m(sg, spec.act_src, [1] * len(spec.act_src))]
    return [torch.cat((a, b)) for a, b in zip(cols, mirrored)]


def xbot_l_spec():
    from types import SimpleNamespace
    from humanoid.utils.symmetry import xbot_l_mirror
    return xbot_l_mirror(SimpleNamespace(env=SimpleNamespace(frame_stack=15, c_frame_stack=3, num_single_obs=47, single_num_privileged_obs=73,
                                                             num_actions=12), terrain=SimpleNamespace(measure_heights=False)))


# the update harness of tests/test_symmetry_gpu.py
def _alg(monkeypatch, precision, N, T, symmetry, epochs=1):
    from humanoid.algo import PPO
    from humanoid.algo.ppo.actor_critic import ActorCritic
    monkeypatch.setattr(PPO, "precision", precision)
    monkeypatch.setattr(PPO, "symmetry", symmetry)
    torch.manual_seed(21)
    dims = dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128]) if precision == "bf16" else dict(actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    ac = ActorCritic(705, 219, 12, **dims)      # (bf16: XBot-L's widths, which the fused kernels take)
    alg = PPO(ac, num_learning_epochs=epochs, num_mini_batches=2, device=DEV)
    alg.init_storage(N, T, [705], [219], [12])
    return alg


def _fill_rollout(alg, seed):
    """What a rollout leaves: random observation rows, the policy's own outputs for them (and, on the bf16 path, the shadows its launches
    write), random returns and advantages."""
    st = alg.storage
    T = st.num_transitions_per_env
    g = torch.Generator(device=DEV).manual_seed(seed)
    st._obs_all.copy_(torch.randn(st._obs_all.shape, device=DEV, generator=g))
    st._priv_all.copy_(torch.randn(st._priv_all.shape, device=DEV, generator=g))
    with torch.inference_mode():
        for s in range(T):
            alg.act(st._obs_all[s], st._priv_all[s])
            st.step = s + 1
    st.returns.copy_(torch.randn(st.returns.shape, device=DEV, generator=g))
    st.advantages.copy_(torch.randn(st.advantages.shape, device=DEV, generator=g))


def _record_batches(monkeypatch, alg):
    """Every index slice update() hands to hgym.make_batch, and net.grads after every hgym_ppo_grad."""
    import hgym
    idx_log, grad_log = [], []
    make_batch, ppo_grad = hgym.make_batch, alg.net.ppo_grad

    def mb(*a, **k):
        idx_log.append(a[9].clone())
        return make_batch(*a, **k)

    def pg(cfg, batch):
        ppo_grad(cfg, batch)
        grad_log.append(alg.net.grads.clone())
    monkeypatch.setattr(hgym, "make_batch", mb)
    monkeypatch.setattr(alg.net, "ppo_grad", pg)
    return idx_log, grad_log
