"""The PPO loss head, sample by sample: a probe network that makes the head's per-sample gradients observable, a float64 autograd
reference, and the case table of tests/test_loss_head.py (host) and tests/test_loss_head_gpu.py (-m gpu).  Plain helpers, no pytest hooks.

The probe.  hgym_ppo_grad returns parameter gradients only.  With one-hot input rows (obs[i] = priv[i] = e_i), hidden layers
W = [I 0; 0 0], b = 0 (ELU keeps 0 and 1 exactly, in fp32 and in bf16) and the head weights W_head[j, i] = mu_target[i, j],
W_critic_head[0, i] = v_target[i] (bf16-representable values), every path computes mu[i] = mu_target[i] and V[i] = v_target[i] EXACTLY (one
non-zero product, fp32 accumulation): clip indicators cannot differ between a kernel and the reference.  The head weight gradient is a
sum with one non-zero term: dW_head[j, i] = g_mu[i, j], dW_critic_head[0, i] = d_v[i] (after one bf16 rounding where dZ is stored as
bf16).  The head biases give sum_i g_mu[i, :] and sum_i d_v[i], the std gradient sum_i g_sigma[i, :], and opt_state[3], [4], [5], [8] the
surrogate, value loss, entropy and KL.

Tolerances (none of them tuned on a kernel's output).
  * fp32 arithmetic of the head.  L_i = sum_j (d^2 / 2s^2 + |log s| + log(2 pi) / 2) + |lp_old| is the condition number of
    exp(lp - lp_old).  The unit of error of a per-sample quantity x_i with A components is  u(x_i) = 2^-24 * (1 + L_i) * max_j |x_i[j]|
    for what passes through the ratio (g_mu, g_sigma, the surrogate), and 2^-24 * |x_i| (no L factor, which is the tighter choice) for
    the value side (d_v, the value loss); the entropy and the KL, sums of A terms that may cancel, take 2^-24 * sum_j |terms|.
    K_REF is the worst error, in these units, of oracle/ppo_oracle.py EVALUATED IN FP32 ON THE CPU against the float64 autograd
    reference, over every per-sample g_mu and d_v of the whole table below (tests/test_loss_head.py recomputes it and compares).
    The GPU bar is GPU_FACTOR * K_REF units with GPU_FACTOR = 8: the kernels add the log-prob terms in another order (4 per lane, then
    two shuffles, in the fused head), contract multiply-adds differently and use the device expf / logf, each good to a few ulp; 8x covers
    that and is orders of magnitude below the effect of one wrong indicator or tie weight (of the size of the gradient itself).
  * bf16 paths store the head gradient as bf16: + 2^-8 * |ref| per stored element (bf16 unit roundoff).  The fused head forms the head
    bias and std sums from the fp32 values before that rounding, and ppo_loss_kernel the std sum: those keep the fp32 bar.  On the
    layer-by-layer bf16 path the two head bias gradients are rowsum_kernel's sums of the STORED (rounded) values, so their bar carries
    the 2^-8 term of every summand.
  * sums over the batch:  sum_i bar_i + B * 2^-24 * sum_i |term_i|.
  * exact ties need no tolerance: the tie weight 0.5 differs from either neighbour by the size of the gradient.

Classes of the table.  `strict` samples lie at least 1e-3 (in log ratio) from log(1 +- clip) and away from every value-loss tie unless
the tie is exact in fp32 AND in float64: every implementation must take the reference's branch.  `rbound` cases (cases of their own) put
the fp32 ratio on the bound itself and at its 1, 2, 4 ulp neighbours: there a result must equal one of the two float64 gradients
(indicator in / out), the same for all components of a sample.  Storage rows that the index list does not select are NaN in every float
column.
"""
import math

import numpy as np
import torch

from oracle import ppo_oracle as P

U24 = 2.0 ** -24
U8 = 2.0 ** -8           # bf16 unit roundoff (8 significand bits, round to nearest)
K_REF = 1.84             # worst fp32-oracle error in units (module docstring); tests/test_loss_head.py::test_k_ref recomputes it
GPU_FACTOR = 8.0
STRICT_MARGIN = 1e-3     # |log ratio - log(1 +- clip)| of every strict sample
MAX_LOG_RATIO = 20.0     # ratio = inf gives 0 * inf = NaN under autograd too: out of scope


def f32(x):
    return float(np.float32(x))


def ppo_constants(clip=0.2, value_coef=1.0, entropy_coef=0.001):
    """The coefficients as the C struct carries them: fp32-rounded (otherwise planted boundaries move)."""
    return dict(clip=f32(clip), value_coef=f32(value_coef), entropy_coef=f32(entropy_coef))


PPO = ppo_constants()
CLIP32 = np.float32(0.2)

# name: (n_obs, n_priv, actor hidden, critic hidden); the widths of tests/test_fused_shapes_gpu.py::ROWS (g1 with a privileged row wide
# enough for one-hot rows of B = 256)
SHAPES = {
    "xbotl": (705, 219, [512, 256, 128], [768, 256, 128]),
    "narrow": (705, 219, [256, 128, 128], [768, 128, 128]),
    "wide3": (705, 219, [512, 256, 256], [512, 256, 384]),
    "g1": (705, 256, [256, 256, 256], [256, 256, 256]),
}
BANDS = {"low": (0.05, 0.3), "mid": (0.75, 1.25), "high": (2.0, 4.0)}
B_XBOTL = (1, 15, 16, 17, 63, 64, 65, 100, 128)
B_G1 = (129, 200, 256)
A_ALL = (1, 3, 4, 5, 8, 10, 11, 12)


def max_batch_of(shape):
    n_obs, n_priv, ah, ch = SHAPES[shape]
    return min([n_obs, n_priv] + list(ah) + list(ch))


# ------------------------------------------------------------------------------------------------ probe
def probe_params(n_obs, n_priv, A, actor_hidden, critic_hidden, mu_target, v_target, std):
    """-> (oracle Params, obs (B, n_obs), priv (B, n_priv)): the one-hot rows and the network that maps row i to mu_target[i], v_target[i]."""
    B = mu_target.shape[0]
    assert mu_target.shape == (B, A) and v_target.shape == (B,)
    assert B <= min([n_obs, n_priv] + list(actor_hidden) + list(critic_hidden))
    for t in (mu_target, v_target):
        assert torch.equal(t.float().to(torch.bfloat16).float(), t.float()), "planted values must be bf16-representable"

    def trunk(k, hidden):
        layers = []
        for n in hidden:
            W = torch.zeros(n, k)
            W[:B, :B] = torch.eye(B)
            layers.append((W, torch.zeros(n)))
            k = n
        return layers, k

    actor, ka = trunk(n_obs, actor_hidden)
    critic, kc = trunk(n_priv, critic_hidden)
    Wa = torch.zeros(A, ka)
    Wa[:, :B] = mu_target.float().t()
    Wc = torch.zeros(1, kc)
    Wc[0, :B] = v_target.float()
    actor.append((Wa, torch.zeros(A)))
    critic.append((Wc, torch.zeros(1)))
    obs, priv = torch.zeros(B, n_obs), torch.zeros(B, n_priv)
    obs[:, :B] = torch.eye(B)
    priv[:, :B] = torch.eye(B)
    return P.Params(actor, critic, std.float().clone()), obs, priv


# ------------------------------------------------------------------------------------------------ float64 autograd reference
def reference(rows, mu, v, std, ppo=PPO, unclipped=False):
    """float64 torch.autograd of the reference's loss (ppo.py:128-168) written out plainly, differentiated w.r.t. mu (B, A), V (B,) and a
    per-sample copy of std (B, A).  rows: dict of the gathered columns actions, values, adv, returns, logp, mu_old, sigma_old.
    Per-sample results (the batch means' 1/B included in the gradients): g_mu, d_v, g_sigma, surr, vl, ent, kl, L; and the surrogate
    gradient with the clip indicator forced in (g_mu_in) and forced out (g_mu_out)."""
    d = lambda t: torch.as_tensor(t).double()
    act, vold, adv, ret, lpo, mo, so = (d(rows[k]) for k in ("actions", "values", "adv", "returns", "logp", "mu_old", "sigma_old"))
    B, A = act.shape
    clip, vcoef, ecoef = ppo["clip"], ppo["value_coef"], ppo["entropy_coef"]
    mu = d(mu).clone().requires_grad_()
    v = d(v).clone().requires_grad_()
    sig = d(std).expand(B, A).clone().requires_grad_()
    dist = torch.distributions.Normal(mu, sig)
    logp = dist.log_prob(act).sum(-1)
    ent = dist.entropy().sum(-1)
    kl_terms = torch.log(sig / so + f32(1e-5)), (so ** 2 + (mo - mu) ** 2) / (2.0 * sig ** 2)
    kl = (kl_terms[0] + kl_terms[1] - 0.5).sum(-1)
    ratio = torch.exp(logp - lpo)
    s1 = -adv * ratio
    s2 = -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surr = torch.max(s1, s2)
    if unclipped:
        vl = (ret - v).pow(2)
    else:
        vc = vold + (v - vold).clamp(-clip, clip)
        vl = torch.max((v - ret).pow(2), (vc - ret).pow(2))
    loss = surr.mean() + vcoef * vl.mean() - ecoef * ent.mean()
    g_mu, d_v, g_sig = torch.autograd.grad(loss, (mu, v, sig), retain_graph=True)
    # indicator forced in: the unclamped surrogate; forced out: the ratio taken to lie beyond its nearer bound, where max(s1, s2) keeps
    # s1 only if it is the larger one (above the range: adv < 0; below it: adv > 0) and the clamped operand has no gradient
    (g_in,) = torch.autograd.grad(s1.mean(), mu, retain_graph=True)
    high = (logp - lpo).detach() > 0
    w_out = torch.where(high, adv < 0, adv > 0).double()
    (g_out,) = torch.autograd.grad((w_out * s1).mean(), mu, retain_graph=True)
    with torch.no_grad():
        dd = act - mu
        L = (dd ** 2 / (2 * sig ** 2) + torch.log(sig).abs() + P.HALF_LOG_2PI).sum(-1) + lpo.abs()
        t_ent = ((0.5 + P.HALF_LOG_2PI) + torch.log(sig).abs()).sum(-1)
        t_kl = (kl_terms[0].abs() + kl_terms[1] + 0.5).sum(-1)
    out = dict(g_mu=g_mu, d_v=d_v, g_sigma=g_sig, surr=surr, vl=vl, ent=ent, kl=kl, L=L, t_ent=t_ent, t_kl=t_kl, g_mu_in=g_in,
               g_mu_out=g_out, log_ratio=logp - lpo, logp=logp)
    return {k: t.detach() for k, t in out.items()}


def units(ref):
    """The unit of error of every per-sample quantity (module docstring), (B,) each."""
    cond = U24 * (1.0 + ref["L"])
    return dict(g_mu=cond * ref["g_mu"].abs().amax(-1), g_mu_in=cond * ref["g_mu_in"].abs().amax(-1),
                g_mu_out=cond * ref["g_mu_out"].abs().amax(-1), g_sigma=cond * ref["g_sigma"].abs().amax(-1),
                surr=cond * ref["surr"].abs(), d_v=U24 * ref["d_v"].abs(), vl=U24 * ref["vl"].abs(), ent=U24 * ref["t_ent"],
                kl=U24 * ref["t_kl"])


def excess(got, ref, unit, factor, stored_bf16=False):
    """Per sample: the worst |got - ref| over the sample's components as a fraction of its bar factor * unit (+ 2^-8 |ref| where the
    value is stored as bf16); 0 where got == ref.  <= 1 passes.  With factor = 1 and no bf16 term this is the error in units."""
    got, ref = got.double().reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    bar = factor * unit.unsqueeze(-1).expand_as(ref)
    if stored_bf16:
        bar = bar + U8 * ref.abs()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    return torch.nan_to_num(r, nan=float("inf")).amax(-1)


def mu_excess(got, ref, un, boundary, factor, stored_bf16=False):
    """excess() of the actor head gradient; a boundary sample is held to the nearer of the two float64 gradients (indicator in / out)."""
    strict = excess(got, ref["g_mu"], un["g_mu"], factor, stored_bf16)
    either = torch.minimum(excess(got, ref["g_mu_in"], un["g_mu_in"], factor, stored_bf16),
                           excess(got, ref["g_mu_out"], un["g_mu_out"], factor, stored_bf16))
    return torch.where(boundary, either, strict)


def sum_bar(unit, terms, factor, stored_bf16=False):
    """Bar of sum_i terms[i] (over dim 0) given the per-sample units: sum_i factor * unit_i + B * 2^-24 * sum_i |term_i|, plus the bf16
    rounding of every summand where the sum is formed from stored bf16 values."""
    B = terms.shape[0]
    u = unit if unit.dim() == terms.dim() else unit.unsqueeze(-1).expand_as(terms)
    bar = factor * u.sum(0) + B * U24 * terms.abs().sum(0)
    return bar + U8 * terms.abs().sum(0) if stored_bf16 else bar


# ------------------------------------------------------------------------------------------------ the case table
def _ulp_step(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


def _logp64(act, mu, std):
    a, m, s = act.astype(np.float64), mu.astype(np.float64), std.astype(np.float64)
    return (-((a - m) ** 2) / (2 * s ** 2) - np.log(s) - P.HALF_LOG_2PI).sum(-1)


def value_tie_pairs():
    """Exact ties of the clipped value loss, searched in numpy float32 on a 1/8 grid and kept only where float64 agrees:
    `edge`: (v, v_old) with v - v_old == +-clip exactly (v_in decides; l1 == l2 there as well), `mid`: (v, v_old, ret) outside the clip
    range with ret the midpoint of v and the clipped value, l1 == l2."""
    grid = [np.float32(k / 8.0) for k in range(-16, 17)]
    c32, c64 = CLIP32, float(CLIP32)
    edge, mid = [], []
    for v in grid:
        for sgn in (1.0, -1.0):
            vold = np.float32(v - np.float32(sgn) * c32)
            if np.float32(v - vold) == np.float32(sgn) * c32 and float(v) - float(vold) == sgn * c64:
                edge.append((float(v), float(vold)))
        for vold in grid:
            d32 = np.float32(v - vold)
            if abs(float(v) - float(vold)) <= c64 + 1e-3:
                continue
            vc32 = np.float32(vold + np.clip(d32, -c32, c32))
            vc64 = float(vold) + float(np.clip(float(v) - float(vold), -c64, c64))
            ret = np.float32((np.float32(v) + vc32) * np.float32(0.5))
            l1, l2 = np.float32(v - ret) * np.float32(v - ret), np.float32(vc32 - ret) * np.float32(vc32 - ret)
            e1, e2 = (float(v) - float(ret)) ** 2, (vc64 - float(ret)) ** 2
            if float(vc32) == vc64 and l1 == l2 and e1 == e2 and l1 > 0:
                mid.append((float(v), float(vold), float(ret)))
    return edge, mid


_BULK_PATTERN = ("in", "hi_far", "lo_far", "hi_near_out", "lo_near_out", "hi_near_in", "lo_near_in", "hi_far", "lo_far", "in")


def _log_ratio_target(kind, rng):
    hi, lo = math.log1p(float(CLIP32)), math.log1p(-float(CLIP32))
    near = rng.uniform(1.1e-3, 1.9e-3)       # within 2e-3 of the bound, no closer than 1e-3 (the fp32 rounding of lp_old moves it by < 1e-5)
    if kind == "in":
        return rng.uniform(-0.15, 0.15)
    if kind in ("hi_far", "lo_far"):
        return (1.0 if kind == "hi_far" else -1.0) * rng.uniform(1.2, 1.8)
    if kind == "hi_near_out":
        return hi + near
    if kind == "hi_near_in":
        return hi - near
    if kind == "lo_near_out":
        return lo - near
    if kind == "lo_near_in":
        return lo + near
    raise KeyError(kind)


def make_case(cls, B, A, band, seed, kinds=None):
    """One case: storage of S > B rows (NaN where unselected), a scattered index list, the planted mu / V / std.  Deterministic in its
    arguments.  cls: bulk | vtie | rbound | ratio1."""
    rng = np.random.RandomState(seed)
    lo_b, hi_b = BANDS[band]
    edge, mid = value_tie_pairs()
    if cls == "vtie":
        tie_rows = [(v, vo, v + dr) for v, vo in edge for dr in (0.75, -0.5)] + list(mid)
        B = len(tie_rows)
    S = B + 7 + B // 3
    idx = np.sort(rng.permutation(S)[:B])
    idx = idx[rng.permutation(B)]                         # scattered and unordered, never a prefix
    std = rng.uniform(lo_b, hi_b, A).astype(np.float32)
    mu = (rng.randint(-32, 33, (B, A)) / 16.0).astype(np.float32)
    v = (rng.randint(-32, 33, B) / 8.0).astype(np.float32)
    if cls == "vtie":
        v = np.array([t[0] for t in tie_rows], dtype=np.float32)
    act = (mu + std * np.clip(rng.randn(B, A), -2.5, 2.5).astype(np.float32)).astype(np.float32)
    so = rng.uniform(lo_b, hi_b, (B, A)).astype(np.float32)
    mo = (mu + std * rng.randn(B, A).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    lp64 = _logp64(act, mu, std)
    adv = (np.where(rng.rand(B) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 2, B)).astype(np.float32)
    # value side, strict: |V - V_old| on both sides of clip and >= 1e-2 away from it; returns away from the midpoint tie
    delta = rng.choice([0.05, 0.15, 0.19, 0.21, 0.3, 1.0], B) * rng.uniform(0.98, 1.02, B) * np.where(rng.rand(B) < 0.5, -1.0, 1.0)
    vold = (v - delta).astype(np.float32)
    ret = (v + rng.randn(B)).astype(np.float32)
    c64 = float(CLIP32)
    for i in range(B):
        for _ in range(64):
            vc = float(vold[i]) + min(max(float(v[i]) - float(vold[i]), -c64), c64)
            if abs(abs(float(v[i]) - float(ret[i])) - abs(vc - float(ret[i]))) >= 1e-3 or abs(float(v[i]) - float(vold[i])) <= c64:
                break
            ret[i] = np.float32(ret[i] + np.float32(0.0625))
    boundary = np.zeros(B, dtype=bool)
    if cls == "bulk":
        if kinds is None:
            kinds = [_BULK_PATTERN[i % len(_BULK_PATTERN)] for i in range(B)]
            kinds = [kinds[i] for i in rng.permutation(B)]
            zero = rng.permutation(B)[:3 + B // 16]
            adv[zero] = 0.0
        lr = np.array([_log_ratio_target(k, rng) for k in kinds])
        lpo = (lp64 - lr).astype(np.float32)
    elif cls == "vtie":
        kinds = ["in"] * B
        lpo = (lp64 - rng.uniform(-0.1, 0.1, B)).astype(np.float32)
        vold = np.array([t[1] for t in tie_rows], dtype=np.float32)
        ret = np.array([t[2] for t in tie_rows], dtype=np.float32)
    elif cls == "rbound":
        # the bound where the indicator decides the gradient: above the range with adv > 0, below it with adv < 0.  |adv| is a power of
        # two, so that s1 = -adv * ratio and s2 = -adv * clamp(ratio) are exact: with any other advantage the two products can round to
        # the same fp32 number while the ratio is an ulp outside the range, and the reference's own rule (torch.max splits the tie, clamp
        # passes nothing) then gives HALF the gradient in fp32 -- a third outcome that float64 does not have
        kinds = []
        lpo = np.zeros(B, dtype=np.float32)
        steps = (0, 1, -1, 2, -2, 4, -4)
        for i in range(B):
            high = (i // len(steps)) % 2 == 0
            bound = math.log1p(float(CLIP32)) if high else math.log1p(-float(CLIP32))
            lpo[i] = _ulp_step(np.float32(lp64[i] - bound), steps[i % len(steps)])
            adv[i] = np.float32((1.0 if high else -1.0) * 2.0 ** rng.randint(-1, 2))
            kinds.append("hi_bound" if high else "lo_bound")
        boundary[:] = True
    elif cls == "ratio1":
        kinds = ["one"] * B
        t = lambda a: torch.from_numpy(a)
        lpo = P.gaussian_log_prob(t(act), t(mu), t(mu) * 0.0 + t(std)).numpy().astype(np.float32)    # the fp32 log-prob itself
        adv = np.where(adv == 0, np.float32(1.0), adv).astype(np.float32)
    else:
        raise KeyError(cls)
    assert np.all(np.abs(lp64 - lpo.astype(np.float64)) <= MAX_LOG_RATIO)

    def store(x):
        out = np.full((S,) + x.shape[1:], np.nan, dtype=np.float32)
        out[idx] = x
        return torch.from_numpy(out)

    return dict(name="%s-B%d-A%d-%s-s%d" % (cls, B, A, band, seed), cls=cls, B=B, A=A, S=S, band=band, kinds=list(kinds),
                idx=torch.from_numpy(idx.astype(np.int64)), std=torch.from_numpy(std), mu=torch.from_numpy(mu), v=torch.from_numpy(v),
                boundary=torch.from_numpy(boundary),
                cols=dict(actions=store(act), values=store(vold), adv=store(adv), returns=store(ret), logp=store(lpo), mu_old=store(mo),
                          sigma_old=store(so)))


def rows_of(case):
    """The gathered (B, *) columns of a case."""
    return {k: t[case["idx"]] for k, t in case["cols"].items()}


def storage_inputs(case, n_obs, n_priv, obs_rows, priv_rows):
    """(S, n_obs), (S, n_priv) storage with the probe's one-hot rows at idx and NaN elsewhere."""
    obs = torch.full((case["S"], n_obs), float("nan"))
    priv = torch.full((case["S"], n_priv), float("nan"))
    obs[case["idx"]] = obs_rows
    priv[case["idx"]] = priv_rows
    return obs, priv


def _build_table():
    bands = list(BANDS)
    cases, seed = [], 1000
    for n, B in enumerate(B_XBOTL + B_G1):
        if B == 1:      # one sample cannot hold every class: four single-sample cases, one per class
            for kind, a in (("in", 1.5), ("hi_far", 0.25), ("lo_near_out", -3.0), ("hi_near_in", 0.0)):
                seed += 1
                c = make_case("bulk", 1, 12, bands[seed % 3], seed, kinds=[kind])
                c["cols"]["adv"][c["idx"]] = a
                cases.append(c)
            continue
        seed += 1
        cases.append(make_case("bulk", B, 12, bands[n % 3], seed))
    for n, A in enumerate(a for a in A_ALL if a != 12):
        for m, B in enumerate((17, 100)):
            seed += 1
            cases.append(make_case("bulk", B, A, bands[(n + m) % 3], seed))
    for A, band in ((12, "low"), (12, "high"), (5, "mid")):
        seed += 1
        cases.append(make_case("vtie", 0, A, band, seed))
    for A, band in ((12, "low"), (12, "mid"), (12, "high"), (5, "low"), (11, "mid")):
        seed += 1
        cases.append(make_case("rbound", 28, A, band, seed))
    for A, band in ((12, "low"), (12, "mid"), (3, "high")):
        seed += 1
        cases.append(make_case("ratio1", 32, A, band, seed))
    return cases


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = _build_table()
    return _TABLE


def shapes_for(case):
    """The network shapes a case fits (one-hot rows need B <= every width)."""
    return [s for s in SHAPES if case["B"] <= max_batch_of(s)]


def oracle_params(case, dtype, width=None):
    """Probe parameters of the smallest network that holds the case (the oracle does not care about widths), in `dtype`."""
    n = width or max(case["B"], 2)
    p, obs, priv = probe_params(n, n, case["A"], [n, n, n], [n, n, n], case["mu"], case["v"], case["std"])
    cast = lambda layers: [(W.to(dtype), b.to(dtype)) for W, b in layers]
    return P.Params(cast(p.actor), cast(p.critic), p.std.to(dtype)), obs.to(dtype), priv.to(dtype)


def run_oracle(case, dtype, fn=None):
    """oracle/ppo_oracle.py::ppo_loss_and_grads on a case in `dtype`, through the probe network."""
    p, obs, priv = oracle_params(case, dtype)
    r = {k: t.to(dtype) for k, t in rows_of(case).items()}
    fn = fn or P.ppo_loss_and_grads
    with torch.no_grad():
        return fn(p, obs, priv, r["actions"], r["values"], r["adv"], r["returns"], r["logp"], r["mu_old"], r["sigma_old"],
                  clip=PPO["clip"], value_coef=PPO["value_coef"], entropy_coef=PPO["entropy_coef"])
