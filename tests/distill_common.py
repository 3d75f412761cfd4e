"""Shared by tests/test_distillation.py (CPU) and tests/test_distillation_gpu.py (-m gpu): the float64 restatement of one
behaviour-cloning minibatch (hgym_bc_grad), of the Adam step behind it (hgym_ppo_apply with no clip that binds) and of a whole
Distillation.update(); the inputs the GPU cases share.

  bc_loss_and_grads   loss and gradients of every W, b of an MLP for the MSE / Huber regression of its output on `target`, through
                      oracle/ppo_oracle.py's mlp_forward / mlp_backward (quant = bf16 rounding: the bf16-operand model of the kernels).
  Adam64              torch.optim.Adam's defaults in float64 with clip_grad_norm_'s coefficient, over a list of tensors.
  distill_update      Distillation.update() restated: the same slices in the same order, one Adam step each.
  make_case           an MLP, S storage rows of observations and targets of which B are named by idx; every other row is NaN.
"""
import functools
import math

import torch

import fused_batch_common as FB
from oracle import ppo_oracle as P

q64 = FB.q64
LOSS_TYPES = ("mse", "huber")
F32_TOL = 1e-5                      # the layer-by-layer fp32 path against float64, relative to the tensor's largest entry
BF16_TOL = FB.BF16_OPERAND_TOL      # the fused bf16 path against the bf16-operand oracle, per tensor, rel-L2


def bc_terms(e, loss_type, delta):
    """Per-element loss and d loss / d e of the residual e = mu - target (before the mean over B A)."""
    if loss_type == "mse":
        return e * e, 2.0 * e
    assert loss_type == "huber" and delta > 0
    a = e.abs()
    return torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta)), e.clamp(-delta, delta)


def bc_loss_and_grads(layers, obs, target, loss_type="mse", delta=1.0, quant=None, mlp=None):
    """-> (loss, [(dW, db), ...]) in the precision of the inputs.  layers: [(W, b), ...]; obs (B, K), target (B, A).
    mlp: (mlp_forward, mlp_backward) restated for another activation (layer_path_common.restated); default ELU(1)."""
    fwd, bwd = mlp if mlp is not None else (P.mlp_forward, P.mlp_backward)
    with torch.no_grad():
        y, acts, pres = fwd(obs, layers, keep=True, quant=quant)
        e = y - target
        le, ge = bc_terms(e, loss_type, delta)
        n = e.numel()
        return le.sum() / n, bwd(ge / n, layers, acts, pres, quant=quant)


def flat(grads):
    return [t for wb in grads for t in wb]


class Adam64:
    """torch.optim.Adam defaults (betas 0.9 / 0.999, eps 1e-8) preceded by clip_grad_norm_(max_norm), all in float64."""

    def __init__(self, tensors):
        self.m = [torch.zeros_like(t) for t in tensors]
        self.v = [torch.zeros_like(t) for t in tensors]
        self.t = 0

    def step(self, tensors, grads, lr, max_norm=None, b1=0.9, b2=0.999, eps=1e-8):
        self.t += 1
        coef = 1.0
        if max_norm is not None:
            total = math.sqrt(sum(float((g * g).sum()) for g in grads))
            coef = min(max_norm / (total + 1e-6), 1.0)
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        out = []
        for w, g, m, v in zip(tensors, grads, self.m, self.v):
            g = g * coef
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            out.append(w - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps))
        return out


def distill_update(layers, obs, target, N, gradient_length, epochs, lr, loss_type="mse", delta=1.0, opt=None, quant=None, max_norm=None):
    """Distillation.update() on (T N, .) rows in float64: for each epoch, for each slice of gradient_length steps in storage order, one
    gradient and one Adam step.  -> (new layers, [loss of every step], the optimiser)."""
    tensors = flat(layers)
    opt = Adam64(tensors) if opt is None else opt
    mb, losses = gradient_length * N, []
    assert obs.shape[0] % mb == 0
    for _ in range(epochs):
        for k in range(obs.shape[0] // mb):
            cur = [(tensors[2 * i], tensors[2 * i + 1]) for i in range(len(tensors) // 2)]
            loss, grads = bc_loss_and_grads(cur, obs[k * mb:(k + 1) * mb], target[k * mb:(k + 1) * mb], loss_type, delta, quant)
            losses.append(float(loss))
            tensors = opt.step(tensors, flat(grads), lr, max_norm)
    return [(tensors[2 * i], tensors[2 * i + 1]) for i in range(len(tensors) // 2)], losses, opt


# ------------------------------------------------------------------------------------------------ inputs
# name: (precision, actor dims input .. head, critic dims) -- "g1" is the smallest net the fused path accepts, "xbotl" the XBot-L actor,
# "ragged" a three-layer fp32 net of widths that are multiples of nothing (the layer-by-layer path), "ragged_bf16" the same in bf16
NETS = {
    "g1": ("bf16", [141, 256, 128, 128, 12], [219, 256, 128, 128, 1]),
    "xbotl": ("bf16", [705, 512, 256, 128, 12], [219, 768, 256, 128, 1]),
    "ragged": ("f32", [47, 40, 24, 12], [19, 24, 1]),
    "ragged_bf16": ("bf16", [47, 40, 24, 12], [19, 24, 1]),             # bf16 operands on the layer-by-layer path (bc_loss_kernel<bf16>)
    "g1_tanh": ("bf16", [141, 256, 128, 128, 12], [219, 256, 128, 128, 1]),      # the fused tiles with a resolved activation (GA kernels)
}
FUSED = ("g1", "xbotl", "g1_tanh")      # the nets the fused bf16 kernels take
TANH = ("g1_tanh",)                     # nn.Tanh() with HgymNetConfig.fused_activation = 1; every other net: ELU(1)


def activation(name):
    import torch.nn as nn
    return nn.Tanh() if name in TANH else None


def mlp_fns(name):
    """(mlp_forward, mlp_backward) of the net's activation: oracle/ppo_oracle.py's for ELU(1), layer_path_common's restatement otherwise."""
    if name not in TANH:
        return None
    import layer_path_common as LP
    return LP.restated(activation(name))


BATCHES = [1, 63, 64, 65, 200]      # a single row, both sides of the 64-row tile, several tiles with a ragged last one
MAX_BATCH = 256


@functools.lru_cache(maxsize=None)
def make_layers(name, seed=11):
    """(actor layers, critic layers), fp32, nn.Linear's default init."""
    _, ad, cd = NETS[name]
    g = torch.Generator().manual_seed(seed)
    p = P.Params.random(ad[0], cd[0], ad[-1], ad[1:-1], cd[1:-1], g)
    return p.actor, p.critic


@functools.lru_cache(maxsize=None)
def make_case(name, B, seed=0):
    """dict(obs (S, K), target (S, A), idx (B,), B, S): S = B + 37 storage rows, every row outside idx NaN.  The targets are the net's
    own output plus N(0, 1) noise scaled so that Huber's |e| falls on both sides of delta = 1 (about a third beyond it)."""
    _, ad, _ = NETS[name]
    g = torch.Generator().manual_seed(1000 * seed + B)
    S = B + 37
    obs = torch.randn(S, ad[0], generator=g)
    actor, _ = make_layers(name)
    with torch.no_grad():
        mu = P.mlp_forward(obs, actor)
    target = mu + torch.randn(S, ad[-1], generator=g)
    idx = FB.make_index(B, S, g)
    dead = torch.ones(S, dtype=torch.bool)
    dead[idx] = False
    obs[dead] = float("nan")
    target[dead] = float("nan")
    return dict(obs=obs, target=target, idx=idx, B=B, S=S, name=name)


def reference(name, case, loss_type, delta=1.0):
    """The float64 reference of a case: on bf16-rounded operands for a bf16 net, plain for an fp32 one.  -> (loss, [dW, db, ...])."""
    prec, _, _ = NETS[name]
    actor, _ = make_layers(name)
    idx = case["idx"]
    loss, grads = bc_loss_and_grads(FB.dbl(actor), case["obs"][idx].double(), case["target"][idx].double(), loss_type, delta,
                                    quant=q64 if prec == "bf16" else None, mlp=mlp_fns(name))
    return float(loss), flat(grads)


def rel_max(a, b):
    """max |a - b| relative to the largest entry of b (the fp32 bar's metric)."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))
