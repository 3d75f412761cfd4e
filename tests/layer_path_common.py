"""Shared by tests/test_layer_path_shapes.py (CPU), tests/test_layer_path_shapes_gpu.py and tests/test_activations_gpu.py (-m gpu):
the layer-by-layer net cases, a Python restatement of how csrc/hgym_net.hip dispatches their dense products to gemm_nt_kernel, and the
float64 MLP reference for any hidden activation (oracle/ppo_oracle.py implements ELU(1) only)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

# (num_obs, num_priv, num_actions, actor hidden, critic hidden, activation, auxiliary head (hidden, out, target offset) or None)
CASES = {
    # 8 + 8 layers: 33 parameter segments, SegTable's capacity; widths 1 .. 257 around every padding unit
    "deep": (47, 73, 12, [100, 37, 5, 130, 17, 1, 33], [129, 15, 64, 3, 257, 16, 2], None, None),
    # every width 1; LeakyReLU(0.01)
    "thin": (705, 219, 1, [1], [1], nn.LeakyReLU(0.01), None),
    # widths at the 16 / 32 / 64 padding boundaries +-1; Sigmoid: sigmoid(0) = 0.5, so a write into a pad column would show
    "pad": (3, 5, 5, [17, 33, 31], [31, 65], nn.Sigmoid(), None),
    # wide and ragged: the 128x128 tiles, partial-column epilogues
    "wide": (705, 219, 11, [1000, 257], [769, 129, 63], None, None),
    # 6 + 6 + 4 = 16 layers with a ragged auxiliary head; Tanh
    "with_aux": (47, 73, 7, [100, 37, 5, 130, 17], [129, 15, 64, 3, 257], nn.Tanh(), ([33, 9, 70], 19, 50)),
}
FWD_M = [1, 15, 16, 17, 63, 65, 333, 4097, 20000]
GRAD_B = [1, 16, 33, 333, 4097]
BIG_B = 61440                     # the BASELINE minibatch
BIG_CASES = ("deep", "wide")
# batches past 32 row-sum chunks (4 096 rows in fp32, 8 192 in bf16), where every rowsum_kernel workgroup sums several of them
HUGE_B = {"f32": 140000, "bf16": 270000}
HUGE_CASE = "pad"
SE = {"f32": 32, "bf16": 64}      # stage_elems: the contraction padding unit (hgym_gemm.hpp)
MAX_SPLITS = 32                   # hgym_net.hip MAX_SPLITS = WsLayout.splits


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def net_config(name, precision, max_batch):
    from hgym import make_net_config
    no, npv, A, ah, ch, act, aux = CASES[name]
    kw = {}
    if aux is not None:
        kw = dict(aux_hidden=aux[0], aux_out=aux[1], aux_target_offset=aux[2])
    return make_net_config(no, npv, A, ah, ch, precision, max_batch, activation=act, **kw)


def layers(name):
    """[(net, K, N)] of every layer of the case (actor, critic, auxiliary head)."""
    no, npv, A, ah, ch, _, aux = CASES[name]
    nets = [("actor", [no] + ah + [A]), ("critic", [npv] + ch + [1])]
    if aux is not None:
        nets.append(("aux", [no] + aux[0] + [aux[1]]))
    return [(n, d[i], d[i + 1], i) for n, d in nets for i in range(len(d) - 1)]


# ---------------------------------------------------------------------------------------------- gemm dispatch, restated
def tile(M, N, splits):
    """launch_gemm's tile configuration (hgym_net.hip)."""
    if N <= 16:
        return "128x16"
    if M <= 16:
        return "16x128"
    if cdiv(M, 128) * cdiv(N, 128) * splits >= 192:
        return "128x128"
    return "64x64"


def split_count(K, N, Mp, se):
    """NetBase::split_count for a layer K -> N over contraction padding Mp: (requested after the clamps, launched)."""
    tiles = cdiv(N, 16 if N <= 16 else 128) * cdiv(K, 128)
    sp = min(cdiv(512, tiles), MAX_SPLITS, Mp // se)
    sp = max(sp, 1)
    per = cdiv(Mp // se, sp)
    return sp, cdiv(Mp // se, per)


def rowsum_splits(Mp, precision):
    """NetBase::rowsum_splits: (workgroups per bias row = its slabs, chunks each one sums)."""
    chunks = cdiv(Mp, 4096 if precision == "f32" else 8192)
    per = cdiv(chunks, min(chunks, MAX_SPLITS))
    return cdiv(chunks, per), per


def products(name, precision, batch, grad):
    """Every gemm_nt_kernel launch of a forward (grad=False) or a gradient (grad=True) of the case at this batch:
    [(product, layer, M, N, K, tile, splits requested, splits launched)]."""
    se = SE[precision]
    Mp = rup(batch, se)
    out = []
    for net, K, N, l in layers(name):
        out.append(("forward", (net, l), batch, N, rup(K, se), tile(batch, N, 1), 1, 1))
        if grad:
            req, sp = split_count(K, N, Mp, se)
            out.append(("dW", (net, l), N, K, Mp, tile(N, K, sp), req, sp))
            if l > 0:
                out.append(("dX", (net, l), batch, K, rup(N, se), tile(batch, K, 1), 1, 1))
    return out


# ---------------------------------------------------------------------------------------------- float64 reference, any activation
def act_fns(m):
    """(f(z), f'(z) from y = f(z)) in float64 for the module m (None: ELU(1))."""
    if m is None:
        m = nn.ELU()
    if isinstance(m, nn.SELU):
        a, s = 1.6732632423543772, 1.0507009873554805
    elif isinstance(m, nn.ELU):
        a, s = float(m.alpha), 1.0
    else:
        a = s = None
    if a is not None:
        return (lambda z: s * torch.where(z > 0, z, a * (torch.exp(z) - 1.0)),
                lambda y: torch.where(y > 0, torch.full_like(y, s), y + s * a))
    if isinstance(m, (nn.ReLU, nn.LeakyReLU)):
        sl = 0.0 if isinstance(m, nn.ReLU) else float(m.negative_slope)
        return (lambda z: torch.where(z > 0, z, sl * z), lambda y: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, sl)))
    if isinstance(m, nn.Tanh):
        return torch.tanh, lambda y: 1.0 - y * y
    return torch.sigmoid, lambda y: y * (1.0 - y)


def restated(m):
    """mlp_forward / mlp_backward of oracle/ppo_oracle.py with the activation m in place of ELU(1)."""
    f, df = act_fns(m)

    def mlp_forward(x, layers, keep=False, quant=None):
        q = quant if quant is not None else (lambda t: t)
        h = q(x)
        acts, pres = [h], []
        for i, (W, b) in enumerate(layers):
            z = F.linear(h, q(W), b)
            if i < len(layers) - 1:
                pres.append(z)
                h = q(f(z))
                acts.append(h)
            else:
                h = z
        return (h, acts, pres) if keep else h

    def mlp_backward(dy, layers, acts, pres, quant=None):
        q = quant
        grads = [None] * len(layers)
        g = dy
        for i in reversed(range(len(layers))):
            W, _ = layers[i]
            if q is None:
                grads[i] = (g.t() @ acts[i], g.sum(dim=0))
            else:
                gb = g.sum(dim=0) if i == len(layers) - 1 else None
                g = q(g)
                grads[i] = (g.t() @ acts[i], gb if gb is not None else g.sum(dim=0))
            if i > 0:
                g = (g @ (W if q is None else q(W))) * df(acts[i])
        return grads

    return mlp_forward, mlp_backward
