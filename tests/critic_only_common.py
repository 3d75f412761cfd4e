"""Shared by tests/test_critic_only.py (CPU) and tests/test_critic_only_gpu.py, tests/test_guard_bands_vf_gpu.py (-m gpu): the float64
restatement of one critic-only minibatch (hgym_vf_grad) and the inputs the GPU cases share.

  vf_terms            per-sample value loss and d loss / d v: clipped (ties of the max split evenly, the clamp passes gradient on the
                      closed range -- torch's backward) and unclipped.
  vf_loss_and_grads   the mean loss and value_coef times its gradient in every W, b of the critic, through oracle/ppo_oracle.py's
                      mlp_forward / mlp_backward (quant = bf16 rounding: the bf16-operand model of the kernels).
  make_case           320 stored rows of every column hgym_ppo_grad reads, B of them named by idx; every other row is NaN.
"""
import functools

import torch

import fused_batch_common as FB
from oracle import ppo_oracle as P

q64 = FB.q64
F32_TOL, BF16_TOL = 1e-4, 5e-3      # the update's bars (README): relative L2 against float64
STORED = 320                        # rows of the storage the minibatches are drawn from
BATCHES = [1, 63, 64, 65, 255, 256, 257]      # both sides of the 64-row tile and of the 256-thread loss block
CLIP, VALUE_COEF = 0.2, 0.7

# name: (precision, actor dims input .. head, critic dims, activation)
#   fused       the narrow actor and the smallest critic trunk of tests/test_fused_shapes_gpu.py at its ragged input widths (third width
#               256: the tile reads its loss inputs from memory)
#   fused_tanh  the critic 256-128-128 (the tile stages its loss inputs in LDS) through the any-activation kernels
#   ragged      widths that are multiples of nothing, fp32, the layer-by-layer path; ragged_tanh: the same in bf16 with nn.Tanh()
NETS = {
    "fused": ("bf16", [188, 256, 128, 128, 12], [146, 256, 256, 256, 1], None),
    "fused_tanh": ("bf16", [188, 256, 128, 128, 12], [146, 256, 128, 128, 1], "tanh"),
    "ragged": ("f32", [47, 40, 24, 12], [19, 24, 17, 1], None),
    "ragged_tanh": ("bf16", [47, 40, 24, 12], [19, 24, 17, 1], "tanh"),
}
FUSED = ("fused", "fused_tanh")


def activation(name):
    import torch.nn as nn
    return nn.Tanh() if NETS[name][3] == "tanh" else None


def mlp_fns(name):
    """(mlp_forward, mlp_backward) of the net's activation."""
    if NETS[name][3] is None:
        return P.mlp_forward, P.mlp_backward
    import layer_path_common as LP
    return LP.restated(activation(name))


def bar(name):
    return BF16_TOL if NETS[name][0] == "bf16" else F32_TOL


# ------------------------------------------------------------------------------------------------ the arithmetic
def vf_terms(v, vold, ret, clip, unclipped):
    """-> (loss_b, d loss_b / d v_b) per sample, in the precision of the inputs."""
    if unclipped:
        return (v - ret) ** 2, 2.0 * (v - ret)
    d = v - vold
    vc = vold + d.clamp(-clip, clip)
    l1, l2 = (v - ret) ** 2, (vc - ret) ** 2
    u1 = torch.where(l1 > l2, 1.0, torch.where(l1 == l2, 0.5, 0.0)).to(v.dtype)
    v_in = ((d >= -clip) & (d <= clip)).to(v.dtype)
    return torch.maximum(l1, l2), u1 * 2.0 * (v - ret) + (1.0 - u1) * 2.0 * (vc - ret) * v_in


def vf_loss_and_grads(layers, priv, vold, ret, clip=CLIP, value_coef=VALUE_COEF, unclipped=False, quant=None, mlp=None):
    """-> (mean loss -- unweighted --, [(dW, db), ...] of value_coef * loss).  layers: [(W, b), ...]; priv (B, K); vold, ret (B,)."""
    fwd, bwd = mlp if mlp is not None else (P.mlp_forward, P.mlp_backward)
    with torch.no_grad():
        y, acts, pres = fwd(priv, layers, keep=True, quant=quant)
        lb, gb = vf_terms(y.squeeze(-1), vold, ret, clip, unclipped)
        B = lb.numel()
        return lb.sum() / B, bwd((value_coef / B * gb).unsqueeze(-1), layers, acts, pres, quant=quant)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def make_params(name, seed=21):
    _, ad, cd, _ = NETS[name]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], g)
    p.std = torch.rand(ad[-1], generator=g) * 0.5 + 0.75
    return p


@functools.lru_cache(maxsize=None)
def make_case(name, B, seed=0):
    """dict(cols: the nine storage columns of hgym.make_batch over STORED rows (every row outside idx NaN), target: the cloning target
    column, idx, B).  The old values lie within about one clip range of the current critic's value -- both sides of the value clip and
    both operands of the max are taken, and a row clipped from below has no gradient at all.  The returns lie above the current value,
    R - V in [0.25, 1): the head bias gradient is a plain sum of d V over the rows, and with residuals of both signs it cancels to a
    number whose RELATIVE error says nothing about the kernel (tests/fused_batch_common.py: make_case plants one sign for the same reason)."""
    _, ad, cd, _ = NETS[name]
    p = make_params(name)
    g = torch.Generator().manual_seed(7000 + 100 * seed + B)
    fwd = mlp_fns(name)[0]
    cols = FB.grad_inputs(p, ad[0], cd[0], ad[-1], STORED, g, fwd)
    obs, priv = cols[0], cols[1]
    with torch.no_grad():
        v = fwd(priv, p.critic).squeeze(-1)
        mu = fwd(obs, p.actor)
    cols[3] = v + torch.randn(STORED, generator=g) * CLIP          # old values
    cols[5] = v + 0.25 + 0.75 * torch.rand(STORED, generator=g)    # returns: R - V of one sign (below)
    target = mu + torch.randn(STORED, ad[-1], generator=g)
    idx = FB.make_index(B, STORED, g)
    dead = torch.ones(STORED, dtype=torch.bool)
    dead[idx] = False
    for t in cols + [target]:
        t[dead] = float("nan")
    return dict(cols=[t.contiguous() for t in cols], target=target.contiguous(), idx=idx, B=B, name=name)


@functools.lru_cache(maxsize=None)
def reference(name, B, unclipped=False, seed=0):
    """The float64 reference of a case: on bf16-rounded operands for a bf16 net.  -> (loss, [dW, db, ...] of the critic)."""
    case, p = make_case(name, B, seed), make_params(name)
    idx = case["idx"]
    loss, grads = vf_loss_and_grads(FB.dbl(p.critic), case["cols"][1][idx].double(), case["cols"][3][idx].double(),
                                    case["cols"][5][idx].double(), unclipped=unclipped, quant=q64 if NETS[name][0] == "bf16" else None,
                                    mlp=mlp_fns(name))
    return float(loss), [t for wb in grads for t in wb]


def rel_l2(a, b):
    return FB.rel_l2(a, b)
