"""CPU-only: the network shapes the layer-by-layer path (csrc/hgym_net.hip: ws_layout, GemmPath) refuses and accepts, decided by host code
before anything launches; and which of launch_gemm's tile configurations and split counts the cases of tests/test_layer_path_shapes_gpu.py
reach (a Python restatement of the dispatch, as tests/test_fused_shapes.py restates the fused kernels' LDS budget)."""
import ctypes as C

import pytest

import layer_path_common as LP


def _lib():
    from hgym import _lib as L
    return L


def _cfg(ah=(64, 64), ch=(64, 64), A=12, no=47, npv=73, precision="f32", aux=None):
    from hgym import make_net_config
    kw = {} if aux is None else dict(aux_hidden=aux[0], aux_out=aux[1], aux_target_offset=aux[2])
    return make_net_config(no, npv, A, list(ah), list(ch), precision, 256, **kw)


def _refused(cfg):
    L = _lib()
    ws = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
    msg = L.lib.hgym_last_error().decode()
    pc = int(L.lib.hgym_net_param_count(C.byref(cfg)))
    return ws == -1 and pc == -1, msg


def _linear_params(dims):
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def _nine_layers(cfg, which):
    # make_net_config cannot express 9 layers (dims arrays hold HGYM_MAX_LAYERS + 1 = 9 widths): set the count on the struct
    setattr(cfg, which + "_layers", 9)
    return cfg


REFUSALS = {
    "actor 0 layers": (lambda: _set(_cfg(), "actor_layers", 0), "layer counts 0/3"),
    "critic 0 layers": (lambda: _set(_cfg(), "critic_layers", 0), "layer counts 3/0"),
    "actor 9 layers": (lambda: _nine_layers(_cfg(), "actor"), "layer counts 9/3"),
    "critic 9 layers": (lambda: _nine_layers(_cfg(), "critic"), "layer counts 3/9"),
    "zero actor width": (lambda: _cfg(ah=(64, 0, 64)), "actor layer 1: non-positive layer dim 64 -> 0"),
    "zero critic width": (lambda: _cfg(ch=(0,)), "critic layer 0: non-positive layer dim 73 -> 0"),
    "zero aux width": (lambda: _cfg(aux=([16, 0], 3, 0)), "auxiliary layer 1: non-positive layer dim 16 -> 0"),
    "num_actions 0": (lambda: _cfg(A=0), "num_actions=0"),
    "num_actions 13": (lambda: _cfg(A=13), "num_actions=13"),
    "actor input != num_obs": (lambda: _set_dim(_cfg(), "actor_dims", 0, 46), "inconsistent with num_obs/num_priv/num_actions"),
    "critic input != num_priv": (lambda: _set_dim(_cfg(), "critic_dims", 0, 74), "inconsistent with num_obs/num_priv/num_actions"),
    "actor head != num_actions": (lambda: _set_dim(_cfg(), "actor_dims", 3, 11), "inconsistent with num_obs/num_priv/num_actions"),
    "critic head != 1": (lambda: _set_dim(_cfg(), "critic_dims", 3, 2), "inconsistent with num_obs/num_priv/num_actions"),
    "aux input != num_obs": (lambda: _set_dim(_cfg(aux=([16], 3, 0)), "aux_dims", 0, 48), "input width 48 must be num_obs = 47"),
    "8 + 8 + 1 layers": (lambda: _cfg(ah=[9] * 7, ch=[9] * 7, aux=([], 3, 0)), "8 actor + 8 critic + 1 auxiliary layers exceed 16"),
    "aux targets past the row": (lambda: _cfg(aux=([16], 3, 71)), "targets [71, 74) must lie inside the privileged row of 73"),
    "aux targets before the row": (lambda: _cfg(aux=([16], 3, -1)), "targets [-1, 2) must lie inside the privileged row of 73"),
}


def _set(cfg, field, v):
    setattr(cfg, field, v)
    return cfg


def _set_dim(cfg, field, i, v):
    getattr(cfg, field)[i] = v
    return cfg


@pytest.mark.parametrize("case", list(REFUSALS))
def test_ws_layout_refuses(case):
    """hgym_net_workspace_bytes and hgym_net_param_count give -1, and the last error names the problem."""
    make, text = REFUSALS[case]
    refused, msg = _refused(make())
    assert refused, case
    assert text in msg, (case, msg)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_ws_layout_accepts_the_limits(precision):
    """8 + 8 layers without an auxiliary head (33 parameter segments: SegTable's capacity), 16 layers in total with one, num_actions 1
    and 12: accepted, with exactly nn.Linear's parameter count (+ std)."""
    L = _lib()
    cases = []
    for name in LP.CASES:
        no, npv, A, ah, ch, _, aux = LP.CASES[name]
        cases.append((LP.net_config(name, precision, 4097), A, [[no] + ah + [A], [npv] + ch + [1]] + ([[no] + aux[0] + [aux[1]]] if aux else [])))
    assert LP.CASES["deep"][3].__len__() + 1 == 8 and LP.CASES["deep"][4].__len__() + 1 == 8
    assert sum(len(d) - 1 for d in cases[-1][2]) == 16
    assert {c[1] for c in cases} >= {1, 12}
    for cfg, A, dims in cases:
        want = A + sum(_linear_params(d) for d in dims)
        assert int(L.lib.hgym_net_param_count(C.byref(cfg))) == want
        assert int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))) > 0
        assert int(L.lib.hgym_net_shadow_ld(C.byref(cfg), 0)) == 0        # the layer-by-layer layout
    # 8 + 8 + 1 layers are refused (above); 7 + 8 + 1 = 16 are accepted
    ok = _cfg(ah=[9] * 6, ch=[9] * 7, aux=([], 3, 0))
    assert int(L.lib.hgym_net_param_count(C.byref(ok))) == 12 + _linear_params([47] + [9] * 6 + [12]) + _linear_params([73] + [9] * 7 + [1]) + \
        _linear_params([47, 3])


def test_coverage_map_of_the_gpu_cases():
    """The products the GPU cases launch reach, in both precisions: all four tile configurations of each product (forward, dW, dX), a
    partial-column epilogue (N % 4 != 0, and the dW output's row stride ldcf = K not a multiple of 4), split counts 1 and 32, and a split
    request that the `per` rounding lowers; and rowsum_kernel workgroups that sum one chunk of the batch and several."""
    for precision in ("f32", "bf16"):
        seen = {}
        for name in LP.CASES:
            runs = [(m, False) for m in LP.FWD_M] + [(b, True) for b in LP.GRAD_B]
            if name in LP.BIG_CASES:
                runs.append((LP.BIG_B, True))
            for batch, grad in runs:
                for prod, _, M, N, K, tile, req, sp in LP.products(name, precision, batch, grad):
                    s = seen.setdefault(prod, dict(tiles=set(), ragged=False, splits=set(), lowered=False))
                    s["tiles"].add(tile)
                    s["ragged"] |= N % 4 != 0
                    s["splits"].add(sp)
                    s["lowered"] |= sp < req
        all4 = {"128x16", "16x128", "128x128", "64x64"}
        for prod in ("forward", "dW", "dX"):
            assert seen[prod]["tiles"] == all4, (precision, prod, seen[prod]["tiles"])
            assert seen[prod]["ragged"], (precision, prod)
        assert {1, 32} <= seen["dW"]["splits"], (precision, seen["dW"]["splits"])
        assert seen["dW"]["lowered"], precision
        # rowsum_kernel: one chunk per workgroup up to 32 chunks (B = 61 440), several past them (LP.HUGE_B)
        assert LP.rowsum_splits(LP.rup(LP.BIG_B, LP.SE[precision]), precision) == ((15, 1) if precision == "f32" else (8, 1))
        assert LP.rowsum_splits(LP.rup(LP.HUGE_B[precision], LP.SE[precision]), precision) == ((18, 2) if precision == "f32" else (17, 2))


def test_split_count_restatement_examples():
    """Spot values of the restated split_count: a 17 -> 33 layer asks for 32 splits; at B = 61 440 in fp32 (1 920 stages) 1 000 x 705
    asks for 11 and gets 11 (per = 175); 3 stages cannot carry 11 requests: one stage each."""
    assert LP.split_count(17, 33, 61440, 32) == (32, 32)
    assert LP.split_count(705, 1000, 61440, 32) == (11, 11)
    assert LP.split_count(705, 1000, 96, 32) == (3, 3)
    # a request the rounding lowers: B = 4 097 in fp32 is 129 stages; 32 requested -> per = 5 -> 26 launched
    assert LP.split_count(47, 100, 4128, 32) == (32, 26)
