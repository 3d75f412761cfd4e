"""Shared by tests/test_fused_batch_edges.py (CPU) and tests/test_fused_batch_edges_gpu.py (-m gpu): the batch dimension of the fused
bf16 update (mlp_fb_kernel / mlp_fb_act_kernel -> dw_kernel_rs with the loss-scalar workgroup -> reduce_slabs_kernel).

  plan(B)       a Python restatement of how FusedPath::grad, FusedPath::dw (csrc/hgym_net.hip), dw_kernel_rs and ppo_scalars_block
                (csrc/hgym_fused.hpp) cut a minibatch of B rows into update tiles, 32-row steps, batch splits, pipeline revolutions and
                summation chains.  Its constants are read out of the two sources by the lines that define them (source_constants) and pinned.
  BATCHES       the minibatch sizes that reach every class of that plan (tests/test_fused_batch_edges.py asserts it through plan()).
  make_case     "spotlit" inputs: the suite's random gradient recipe, with the rows under test -- the tail of the last step, the head of
                the last split, the first row -- made unclipped and heavy, so that they carry a known share of every tensor's gradient.
  oracle_grad, removed_spot, tensor_errors
                the float64 bf16-operand reference, the same gradient without the spot rows' contribution, and the comparison the GPU
                test asserts (rel-L2 per parameter tensor).

Why spotlit: with random inputs one row of a minibatch of 3137 carries 0.4 - 0.8 % of a tensor's gradient norm -- the size of the 5e-3
bar -- and a clipped row carries nothing of the actor's, so a kernel that dropped or doubled the last step of the last split would pass."""
import functools
import math
import os
import re

import torch

from oracle import ppo_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "humanoid-gym_amd", "csrc")

# ------------------------------------------------------------------------------------------------ the constants, from the sources
# name: (file, regular expression over the defining line with one group per number, the pinned numbers)
SOURCE_LINES = {
    "tile_rows": ("hgym_net.hip", r"const int tiles = \(int\)round_up\(B, (\d+)\) / (\d+);", (64, 64)),
    "pad_rows": ("hgym_net.hip", r"const int Bp = \(int\)round_up\(B, (\d+)\);", (64,)),
    "step_rows": ("hgym_net.hip", r"d\.steps_total = Bp / (\d+);", (32,)),
    "step_rows_idx": ("hgym_fused.hpp", r"int mrow = \(step0 \+ \(t < nsteps \? t : nsteps - 1\)\) \* (\d+) \+ irow;", (32,)),
    "dw_splits": ("hgym_net.hip", r"w->dw_splits = (\d+);", (8,)),
    "steps_per_split": ("hgym_net.hip", r"d\.steps_per_split = ceil_div\(d\.steps_total, w\.dw_splits\);", ()),
    "unroll": ("hgym_fused.hpp", r"const int np = \(nsteps \+ (\d+)\) / (\d+) \* (\d+);", (5, 6, 6)),
    "unroll_loop": ("hgym_fused.hpp", r"for \(int t0 = 0; t0 < np; t0 \+= (\d+)\) \{", (6,)),
    "chains": ("hgym_fused.hpp", r"for \(int part = tid / LOSS_PARTIALS; part < (\d+); part \+= nthreads / LOSS_PARTIALS\)", (16,)),
    "chain_body": ("hgym_fused.hpp", r"for \(; b \+ (\d+) < nblocks; b \+= (\d+)\) \{", (48, 64)),
    "chain_rest": ("hgym_fused.hpp", r"for \(; b < nblocks; b \+= (\d+)\) s0 \+= \(double\)partials", (16,)),
    "scal_group": ("hgym_net.hip", r"ppo\.lr_max, (\d+), grad_sigma\(\)\};", (1,)),      # ScalArgs::group of the fused path: one row per tile
}
TILE, STEP, SPLITS, UNROLL, CHAINS, CHAIN_BODY = 64, 32, 8, 6, 16, 48
RE_DERIVE = ("the batch plan of the fused update changed (%s): re-derive tests/fused_batch_common.py's plan() and BATCHES from "
             "FusedPath::grad / FusedPath::dw / dw_kernel_rs / ppo_scalars_block before pinning the new value")


def source_constants():
    """{name: tuple of ints} read from csrc by SOURCE_LINES; a defining line that is gone or occurs with two values raises."""
    text, out = {}, {}
    for name, (fn, rx, _) in SOURCE_LINES.items():
        if fn not in text:
            with open(os.path.join(CSRC, fn)) as f:
                text[fn] = f.read()
        found = {m.groups() for m in re.finditer(rx, text[fn])}
        if len(found) != 1:
            raise AssertionError(RE_DERIVE % ("%s: %d distinct matches of %r in %s" % (name, len(found), rx, fn)))
        out[name] = tuple(int(v) for v in found.pop())
    return out


# ------------------------------------------------------------------------------------------------ the plan
def _cdiv(a, b):
    return -(-a // b)


def chain_loops(nblocks):
    """ppo_scalars_block's 16 strided chains over `nblocks` partial rows: [(passes of the 4-way body, passes of the remainder loop)]."""
    out = []
    for part in range(CHAINS):
        b, body, rest = part, 0, 0
        while b + CHAIN_BODY < nblocks:
            b += CHAIN_BODY + CHAINS
            body += 1
        while b < nblocks:
            b += CHAINS
            rest += 1
        out.append((body, rest))
    return out


def plan(B):
    """What the fused update does with a minibatch of B rows (the names are the kernels')."""
    assert B >= 1
    tiles = _cdiv(B, TILE)                                  # FusedPath::grad: update tiles, the last one ragged
    steps_total = tiles * TILE // STEP                      # FusedPath::dw: Bp / 32
    sps = _cdiv(steps_total, SPLITS)
    nsteps = [min(steps_total - s * sps, sps) for s in range(SPLITS)]       # dw_kernel_rs, as computed: <= 0 on an empty split
    assert min(nsteps) >= -(UNROLL - 1)                     # (nsteps + 5) / 6 never divides a negative number
    np_ = [(n + UNROLL - 1) // UNROLL * UNROLL for n in nsteps]
    last_step = (B - 1) // STEP                             # the last step that holds a valid row
    used = sum(1 for n in nsteps if n > 0)
    # valid rows per split (the last used split may hold steps that are all padding: B <= 32 leaves split 1 with one such step)
    rows = [max(0, min(B, (s * sps + max(n, 0)) * STEP) - s * sps * STEP) for s, n in enumerate(nsteps)]
    return dict(B=B, tiles=tiles, steps_total=steps_total, steps_per_split=sps, nsteps=nsteps, np=np_, used_splits=used,
                last_step=last_step, tail_rows=B - last_step * STEP, last_split=last_step // sps, split_rows=rows,
                padding_steps=steps_total - 1 - last_step, nblocks=tiles, chains=chain_loops(tiles))


BATCHES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 289, 333, 448, 449, 577, 700, 705, 800, 1024, 1025, 1090, 1290, 1570,
           3072, 3073, 3137, 4096, 4097, 4161]
REDUCED = [1, 33, 65, 577, 1090, 3073]                      # the other kernels of the family, spot "tail"
SPOTS = ("tail", "split_head", "row0")


def spot_positions(B, spot):
    """Batch positions of the rows a spot names."""
    pl = plan(B)
    if spot == "tail":
        return list(range(pl["last_step"] * STEP, B))
    if spot == "split_head":
        first = pl["last_split"] * pl["steps_per_split"] * STEP
        return list(range(first, min(first + STEP, B)))
    assert spot == "row0"
    return [0]


def spots_of(B):
    """The spots that exist at B: those that name another set of rows than the ones before them."""
    out, seen = [], []
    for s in SPOTS:
        pos = spot_positions(B, s)
        if pos not in seen:
            seen.append(pos)
            out.append(s)
    return out


CASES = [(B, s) for B in BATCHES for s in spots_of(B)]

# ------------------------------------------------------------------------------------------------ the bar
BF16_OPERAND_TOL = 5e-3      # fused kernels vs the bf16-operand oracle, per tensor, rel-L2 (tests/test_fused_shapes_gpu.py)
BARS = {}                    # B: its own bar, where 5e-3 does not hold for a stated reason (with the measured value beside it)
SHARE_FACTOR = 10.0          # a spot carries at least this many bars of every tensor but std


def bar_for(B):
    return BARS.get(B, BF16_OPERAND_TOL)


# ------------------------------------------------------------------------------------------------ nets
# name: (num_obs, num_priv, num_actions, actor hidden, critic hidden); tests/test_fused_shapes_gpu.py ROWS
SHAPES = {
    "xbotl": (705, 219, 12, [512, 256, 128], [768, 256, 128]),
    "g1": (705, 219, 12, [256, 256, 256], [256, 256, 256]),        # fb_body<1>, `pre` gather off
    "a10": (705, 219, 10, [512, 384, 128], [512, 512, 128]),       # A = 10: the scalar loss branch
}
NAMES = ["std"] + ["%s.%d.%s" % (n, l, k) for n in ("actor", "critic") for l in (0, 2, 4, 6) for k in ("weight", "bias")]
MAX_BATCH = 4224             # 66 tiles: the largest B of BATCHES


def q64(t):
    """bf16 round-to-nearest-even, kept in the tensor's own precision (the float64 oracle)."""
    return t.to(torch.bfloat16).to(t.dtype)


def dbl(layers):
    return [(W.double(), b.double()) for W, b in layers]


@functools.lru_cache(maxsize=None)
def make_params(shape, seed=5):
    no, npv, A, ah, ch = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(no, npv, A, ah, ch, g)
    p.std = torch.rand(A, generator=g) * 0.5 + 0.75
    return p


class _oracle_mlp:
    """oracle/ppo_oracle.py implements ELU(1); under another activation its two MLP functions are swapped for the restated ones
    (layer_path_common.restated) while the reference runs."""

    def __init__(self, fns):
        self.fns = fns

    def __enter__(self):
        self.keep = (P.mlp_forward, P.mlp_backward)
        if self.fns is not None:
            P.mlp_forward, P.mlp_backward = self.fns

    def __exit__(self, *exc):
        P.mlp_forward, P.mlp_backward = self.keep


# ------------------------------------------------------------------------------------------------ spotlit inputs
FACTOR_0 = 0.3      # spot weight = max(1, FACTOR_0 * sqrt(B / rows in the spot)): see weight_factor


def weight_factor(B, n_spot):
    """n of B rows with gradients of the same size and independent directions carry sqrt(n / B) of a tensor's norm; the spot rows'
    advantage and value residual are `factor` times a magnitude in [1, 2] where the other rows have |N(0, 1)| and (for the actor) about
    half of them are clipped to nothing.  FACTOR_0 * sqrt(B / n) puts the share of every tensor between 0.05 (asserted on the host) and
    about one half: heavy enough to be seen, not so heavy that the other rows stop counting in the same case."""
    return max(1.0, FACTOR_0 * math.sqrt(B / n_spot))


def grad_inputs(p, n_obs, n_priv, A, S, g, fwd=P.mlp_forward):
    """tests/test_fused_shapes_gpu.py's _grad_inputs: the nine batch columns over S storage rows, old log-probabilities near the current
    policy's so that ratios fall on both sides of the clip range."""
    obs, priv = torch.randn(S, n_obs, generator=g), torch.randn(S, n_priv, generator=g)
    act, mu_o = torch.randn(S, A, generator=g), torch.randn(S, A, generator=g) * 0.3
    sg_o = torch.rand(S, A, generator=g) * 0.5 + 0.75
    val, adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    with torch.no_grad():
        mu_now = fwd(obs, p.actor)
    lp_o = P.gaussian_log_prob(act, mu_now, mu_now * 0 + p.std) + torch.randn(S, generator=g) * 0.3
    return [obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o]


def make_index(B, S, g):
    """B storage rows out of S > B: a permutation prefix that contains row 0 and row S - 1 (B = 1: row S - 1 alone) and, from B = 3 on,
    one row twice (B = 2 has room for the two end rows only)."""
    assert S > B
    if B == 1:
        return torch.tensor([S - 1], dtype=torch.int64)
    distinct = B if B < 3 else B - 1
    inner = (torch.randperm(S - 2, generator=g) + 1)[:distinct - 2].tolist()
    rows = inner + [0, S - 1]
    order = torch.randperm(distinct, generator=g).tolist()
    rows = [rows[i] for i in order]
    if distinct < B:
        src = int(torch.randint(distinct, (1,), generator=g))
        at = int(torch.randint(distinct + 1, (1,), generator=g))
        rows.insert(at, rows[src])
    return torch.tensor(rows, dtype=torch.int64)


def make_case(B, spot, seed, shape="xbotl", mlp=None, clip=0.2, aux_target=None):
    """-> dict(cols: the nine storage columns (S rows; every row outside idx is NaN), idx, spot_pos: the batch positions that hold a spot
    row (a repeated row counts at both), factor, B, S).  mlp: (mlp_forward, mlp_backward) restated for another activation.

    On the spot rows the old log-probability is the current policy's (float64 on bf16 operands, what the oracle forms), so the ratio is 1
    up to the kernels' bf16 error and the surrogate is unclipped; the old value lies within clip / 4 of the current one, so the value
    clip is inactive; advantage = +-factor * [1, 2) and returns - V = factor * [1, 2) (one sign: the critic's head bias gradient, a
    plain sum over the rows, does not cancel among them).  aux_target = (offset, width): the columns of the privileged row an auxiliary
    head regresses; its loss is an unweighted MSE, so the spot rows are made heavy for it by scaling those targets by 2 * factor (before
    the critic's current value is taken from the row)."""
    no, npv, A, _, _ = SHAPES[shape]
    p = make_params(shape)
    g = torch.Generator().manual_seed(seed)
    S = B + 37
    fwd = mlp[0] if mlp is not None else P.mlp_forward
    cols = grad_inputs(p, no, npv, A, S, g, fwd)
    idx = make_index(B, S, g)
    rows = sorted({int(idx[i]) for i in spot_positions(B, spot)})
    spot_pos = [i for i in range(B) if int(idx[i]) in rows]
    factor = weight_factor(B, len(spot_pos))
    obs, priv, act, val, adv, ret, lp_o, mu_o, sg_o = cols
    R = torch.tensor(rows, dtype=torch.int64)
    if aux_target is not None:
        off, width = aux_target
        priv[R, off:off + width] *= 2.0 * factor
    with torch.no_grad():
        mu = fwd(obs[R].double(), dbl(p.actor), quant=q64)
        v = fwd(priv[R].double(), dbl(p.critic), quant=q64).squeeze(-1)
    n = len(rows)
    lp_o[R] = P.gaussian_log_prob(act[R].double(), mu, mu * 0 + p.std.double()).float()
    val[R] = (v + (torch.rand(n, generator=g).double() - 0.5) * (clip / 2)).float()
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    adv[R] = sign * factor * (1.0 + torch.rand(n, generator=g))
    ret[R] = (v + factor * (1.0 + torch.rand(n, generator=g).double())).float()
    dead = torch.ones(S, dtype=torch.bool)
    dead[idx] = False
    for t in cols:
        t[dead] = float("nan")
    return dict(cols=cols, idx=idx, spot_pos=spot_pos, factor=factor, B=B, S=S, spot=spot, shape=shape)


# ------------------------------------------------------------------------------------------------ reference and metric
def oracle_grad(case, positions=None, mlp=None, unclipped=False):
    """oracle/ppo_oracle.py:ppo_loss_and_grads in float64 on bf16-rounded operands, over the minibatch (or over `positions` of it)."""
    p = make_params(case["shape"])
    idx = case["idx"] if positions is None else case["idx"][torch.tensor(positions, dtype=torch.int64)]
    sel = [t[idx].double() for t in case["cols"]]
    if unclipped:       # (R - V)^2: with the old values at the returns l2 <= l1 always (tests/test_fused_activations_gpu.py)
        sel[3] = sel[5].clone()
    pd = P.Params(dbl(p.actor), dbl(p.critic), p.std.double())
    with _oracle_mlp(mlp), torch.no_grad():
        return P.ppo_loss_and_grads(pd, *sel, quant=q64)


def removed_spot(case, want, mlp=None, unclipped=False):
    """The minibatch gradient `want` without what the spot rows add to it: they are n of the B terms of every mean, so their part is
    n / B times the oracle on those rows alone.  (std: that also takes n / B of the entropy term away, which is no row's -- std is
    left out wherever this is used.)"""
    n, B = len(case["spot_pos"]), case["B"]
    alone = oracle_grad(case, case["spot_pos"], mlp, unclipped)
    return [w - (n / B) * a for w, a in zip(want["grads"].tensors(), alone["grads"].tensors())]


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def tensor_errors(got, want):
    """{parameter tensor: rel-L2 of got against want}: what the GPU test holds against bar_for(B), tensor by tensor."""
    assert len(got) == len(want) == len(NAMES)
    return {k: rel_l2(a, r) for k, a, r in zip(NAMES, got, want)}


# ------------------------------------------------------------------------------------------------ auxiliary (denoising) head
@functools.lru_cache(maxsize=None)
def make_head(hidden, out, seed=6):
    g = torch.Generator().manual_seed(seed)
    return P.Params.random(SHAPES["xbotl"][0], 8, out, list(hidden), [8, 8, 8], g).actor


def oracle_head_grad(case, head, off, out, coef, positions=None):
    """The head's coef * MSE against columns [off, off + out) of the privileged row, as tests/test_fused_shapes_gpu.py's
    test_aux_head_gradient_vs_oracle forms it: mlp_backward of dL/dy = 2 coef (y - t) / (B out).  -> ([W, b, ...] gradients, MSE)."""
    idx = case["idx"] if positions is None else case["idx"][torch.tensor(positions, dtype=torch.int64)]
    x, t = case["cols"][0][idx].double(), case["cols"][1][idx].double()[:, off:off + out]
    hd = dbl(head)
    with torch.no_grad():
        y, acts, pres = P.mlp_forward(x, hd, keep=True, quant=q64)
        hg = P.mlp_backward(2.0 * coef * (y - t) / (idx.numel() * out), hd, acts, pres, quant=q64)
    return [t_ for wb in hg for t_ in wb], float(((y - t) ** 2).mean())


# ------------------------------------------------------------------------------------------------ the other kernels of the family
AUX_HEAD = ([512, 256, 256], 73, 219 - 73, 0.5)      # tests/test_fused_shapes_gpu.py AUX_CASES["fused"]: hidden, out, target offset; aux_coef
VARIANTS = ("g1", "a10", "tanh", "unclipped", "aux")


def variant_case(variant, B, spot="tail"):
    """-> (case, keyword arguments of oracle_grad / removed_spot, AUX_HEAD or None) of one row of the reduced list."""
    seed = 2000 + B
    if variant in ("g1", "a10"):
        return make_case(B, spot, seed, shape=variant), {}, None
    if variant == "tanh":
        import torch.nn as nn
        import layer_path_common as LP
        mlp = LP.restated(nn.Tanh())
        return make_case(B, spot, seed, mlp=mlp), dict(mlp=mlp), None
    if variant == "unclipped":
        return make_case(B, spot, seed), dict(unclipped=True), None
    assert variant == "aux"
    return make_case(B, spot, seed, aux_target=(AUX_HEAD[2], AUX_HEAD[1])), {}, AUX_HEAD
