"""-m gpu: the three entry points of value-target normalisation (hgym_value_denormalize, hgym_value_norm_merge, hgym_value_normalize;
include/hgym.h) against the numpy restatement of tests/value_norm_common.py.

  * sizes on either side of every switch: 1, 2, 63, 64, 65 (a wavefront), C - 1, C, C + 1, 2 C + 1 (C = HGYM_VALUE_NORM_CHUNK values per
    workgroup) and G C + 1 (G = HGYM_VALUE_NORM_MAX_BLOCKS: workgroups walk the chunks with a stride), on 16-byte aligned columns (16-byte
    loads) and on columns one float off (4-byte loads);
  * statistics: count exact, mean and var within 1e-10 relative of the restatement (tests/test_rnd_gpu.py's bar for fixed-order fp64
    statistics) on unit-scale inputs with |mean| <= 10 std; every test prints its largest error;
  * the two maps BITWISE what torch fp32 (on the host: IEEE, one rounding per operation) gives from the device's own mean_f and scale_f;
  * mean = 100, std = 0.01: the bound derived below;
  * edge states, aliasing, bad arguments, guard bands."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import guard_common as GC
import value_norm_common as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-10
CH, G = V.CHUNK, V.MAX_BLOCKS
SIZES = (1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1, G * CH + 1)


def _column(n, mean, std, seed, skew=0):
    """n fp32 values mean + std * z on the device -- skew floats past a 256-byte aligned address -- and their host copy."""
    g = torch.Generator().manual_seed(seed)
    host = (mean + std * torch.randn(n, generator=g, dtype=torch.float64)).float()
    store = torch.empty(n + 64 + skew, dtype=torch.float32, device=DEV)
    off = (-store.data_ptr() // 4) % 64 + skew
    dev = store[off:off + n]
    dev.copy_(host)
    assert dev.data_ptr() % 256 == 4 * skew
    return dev, host


def _floats(block, eps):
    """The device's own mean_f and scale_f, from a host copy of its block: (float)mean, (float)sqrt(var) + eps."""
    b = block.cpu()
    return b[1].float(), torch.sqrt(b[2]).float() + torch.tensor(eps, dtype=torch.float32)


def _check_stats(block, want, what):
    got = [float(v) for v in block.cpu()]
    assert got[0] == want[0], (what, got, want)
    err = max(V.rel(got[1], want[1]) if want[1] != 0.0 else abs(got[1]), V.rel(got[2], want[2]) if want[2] != 0.0 else abs(got[2]))
    assert err <= RTOL, (what, got, want, err)
    return err


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("n", SIZES)
def test_statistics_and_maps_at_every_switch(n, skew):
    import hgym
    from hgym import _lib as L
    mean, std = ((0.0, 1.0), (5.0, 1.0), (-10.0, 1.0), (2.0, 0.5))[(n + skew) % 4]      # unit scale, |mean| <= 10 std
    eps = V.EPS
    cols = [_column(n, mean + 0.3 * k, std, 100 * n + 10 * k + skew, skew) for k in range(3)]
    block, scratch = L.value_norm_block(DEV), L.value_norm_scratch(n, DEV)
    assert scratch.numel() == V.scratch_doubles(n)
    state, worst = V.INITIAL, 0.0
    for k, (dev, host) in enumerate(cols):
        hgym.value_norm_merge(dev, block, scratch)
        batch = V.batch_stats(host.numpy())
        state = V.merge(state, batch)
        worst = max(worst, _check_stats(block, state, "merge %d" % k), _check_stats(scratch[:3], batch, "batch %d" % k))
        assert int(scratch.view(torch.int64)[L.VALUE_NORM_TICKET]) == 0      # the arrival counter is left zero
        assert torch.equal(dev.cpu(), host)                                  # the column is only read
        if k == 0:      # from the initial state: exactly the batch's statistics
            assert torch.equal(block.cpu()[1:], scratch[1:3].cpu()) and float(block[0]) == float(n)
    # three merges: the statistics of the concatenation
    worst = max(worst, _check_stats(block, V.batch_stats(np.concatenate([h.numpy() for _, h in cols])), "concatenation"))
    print("n=%d skew=%d: largest relative error of mean / var %.3e" % (n, skew, worst))
    # the maps, bitwise, from the device's own floats
    mean_f, scale_f = _floats(block, eps)
    dev, host = cols[0]
    y = hgym.value_normalize(dev.clone(), block, eps)
    assert torch.equal(y.cpu().view(torch.int32), ((host - mean_f) / scale_f).view(torch.int32))
    want = host * scale_f
    want = want + mean_f
    out = torch.full_like(dev, 777.0)
    hgym.value_denormalize(dev, block, eps, out=out)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(dev.cpu(), host)
    alias = dev.clone()
    hgym.value_denormalize(alias, block, eps)      # dst == src
    assert torch.equal(alias.view(torch.int32), out.view(torch.int32))
    # ... and the restatement's maps from the restatement's state agree with the device's floats whenever the states round alike
    rm, rs = V.floats(tuple(float(v) for v in block.cpu()), eps)
    assert float(rm) == float(mean_f) and float(rs) == float(scale_f)
    assert np.array_equal(V.normalize(host.numpy(), tuple(float(v) for v in block.cpu()), eps).view(np.int32), y.cpu().numpy().view(np.int32))


def test_same_inputs_same_bits_and_the_load_width_does_not_matter():
    import hgym
    from hgym import _lib as L
    n = 37 * CH + 301
    _, host = _column(n, 3.0, 1.0, 4242)
    blocks = []
    scratch = L.value_norm_scratch(n, DEV)
    for skew in (0, 0, 1, 3):
        store = torch.empty(n + 64 + skew, dtype=torch.float32, device=DEV)
        off = (-store.data_ptr() // 4) % 64 + skew
        dev = store[off:off + n]
        dev.copy_(host)
        block = L.value_norm_block(DEV)
        hgym.value_norm_merge(dev, block, scratch)      # the same scratch, never zeroed again
        hgym.value_norm_merge(dev, block, scratch)
        blocks.append(block.cpu().view(torch.int64).clone())
    assert all(torch.equal(b, blocks[0]) for b in blocks), blocks


def test_constant_batch_and_zero_eps():
    import hgym
    from hgym import _lib as L
    for n in (1, CH + 5):
        dev = torch.full((n,), 2.5, dtype=torch.float32, device=DEV)
        block, scratch = L.value_norm_block(DEV), L.value_norm_scratch(n, DEV)
        hgym.value_norm_merge(dev, block, scratch)
        assert [float(v) for v in block.cpu()] == [float(n), 2.5, 0.0]
        y = hgym.value_normalize(dev.clone(), block, V.EPS)
        assert bool((y.view(torch.int32) == 0).all())      # (2.5 - 2.5) / eps = +0
        back = hgym.value_denormalize(y, block, V.EPS)
        assert bool((back == 2.5).all())
        # eps = 0 is accepted; on a varying batch it is the plain standardisation
        dev2, host2 = _column(n + 1, 1.0, 1.0, n)
        b2 = L.value_norm_block(DEV)
        hgym.value_norm_merge(dev2, b2, L.value_norm_scratch(n + 1, DEV))
        mean_f, scale_f = _floats(b2, 0.0)
        assert torch.equal(hgym.value_normalize(dev2.clone(), b2, 0.0).cpu().view(torch.int32), ((host2 - mean_f) / scale_f).view(torch.int32))


def test_ill_conditioned_batch_within_the_derived_bound():
    """mean = 100, std = 0.01 (|mean| = 10^4 std), n = 65 C + 17.  The bound of the chunk-wise two-pass + Chan formulation, u = 2^-53,
    gamma_k = k u / (1 - k u), X = max |x|:

    A chunk's mean is a tree sum of <= 1024 exact fp64 terms (3 roundings in the thread, 6 over the lanes, 3 over the wavefronts) and a
    division: |mean_c~ - mean_c| <= gamma_13 X.  Every Chan step forms mean = mean_a + d * (n_b / n): an average of its children's means
    (whose errors it therefore does not enlarge) plus 3 more roundings of numbers <= X; with L = ceil(chunks / 256) - 1 + 6 + 3 steps on the
    longest path (thread, lanes, wavefronts) every node's mean is within E = gamma_(13 + 3 L) X of the true mean of its values.
    The chunk's M2~ = sum (x - mean_c~)^2 (1 + theta) = (M2_c + n_c e_c^2)(1 + theta), |theta| <= gamma_15 (x - mean_c~, its square, 12 for
    the tree).  With TRUE means, sum_c M2_c + sum_nodes B_node = M2 exactly, B = d^2 w, w = n_a n_b / n, all terms >= 0 (Chan's identity,
    telescoped).  A node's computed term uses d~ = d + delta, |delta| <= 2 E: B~ - B = (2 d delta + delta^2) w.  Over all nodes, by
    Cauchy-Schwarz and sum_nodes w <= L n (w <= min(n_a, n_b), every value is in at most one node per step):
        sum w 2 |d| |delta| <= 4 E sqrt(L n) sqrt(M2),        sum w delta^2 <= 4 E^2 L n,
    and each term carries <= 8 roundings per step on its way to the root (d, d^2, n_a n_b, / n, the product, two additions; the terms are
    non-negative, so the factors are relative).  Divided by M2 = n var, with s = sqrt(var):
        |var~ - var| / var <= gamma_(15 + 8 L + 1) + (gamma_13 X / s)^2 + 4 sqrt(L) (E / s) + 4 L (E / s)^2
    (+ 1: the final M2 / n).  The mean: |mean~ - mean| <= E.  The restatement itself (math.fsum, two passes) is within 8 u of the exact
    statistics of the fp32 inputs, which is added.  Here chunks = 66, L = 9, E / s = 4.4e-11: the bound is 5.3e-10 for var and
    4.4e-15 |mean| for the mean -- dominated by 4 sqrt(L) E / s, the price of |mean| = 10^4 std; a sum of raw squares would lose
    10^8 u = 1.1e-8.  Measured on the MI355X: see the printed line, and DESIGN.md section 31."""
    import hgym
    from hgym import _lib as L
    n = 65 * CH + 17
    dev, host = _column(n, 100.0, 0.01, 99)
    block, scratch = L.value_norm_block(DEV), L.value_norm_scratch(n, DEV)
    hgym.value_norm_merge(dev, block, scratch)
    got = [float(v) for v in block.cpu()]
    cnt, mean, var = V.batch_stats(host.numpy())
    u = V.U
    gamma = lambda k: k * u / (1.0 - k * u)
    chunks = (n + CH - 1) // CH
    steps = (chunks + 255) // 256 - 1 + 6 + 3
    X, s = float(host.abs().max()), math.sqrt(var)
    E = gamma(13 + 3 * steps) * X
    bound_var = gamma(15 + 8 * steps + 1) + (gamma(13) * X / s) ** 2 + 4.0 * math.sqrt(steps) * (E / s) + 4.0 * steps * (E / s) ** 2 + 8 * u
    bound_mean = E + 8 * u * abs(mean)
    print("ill-conditioned: var error %.3e relative (bound %.3e), mean error %.3e (bound %.3e)"
          % (V.rel(got[2], var), bound_var, abs(got[1] - mean), bound_mean))
    assert got[0] == cnt and abs(got[1] - mean) <= bound_mean and V.rel(got[2], var) <= bound_var
    # the maps stay finite and bitwise torch's
    mean_f, scale_f = _floats(block, V.EPS)
    y = hgym.value_normalize(dev.clone(), block, V.EPS)
    assert torch.equal(y.cpu().view(torch.int32), ((host - mean_f) / scale_f).view(torch.int32)) and bool(torch.isfinite(y).all())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_bad_arguments_launch_nothing_and_write_nothing():
    from hgym import _lib as L
    n = CH + 3
    x = torch.full((n,), 3.0, dtype=torch.float32, device=DEV)
    dst = torch.full((n,), 777.0, dtype=torch.float32, device=DEV)
    block = torch.tensor([5.0, 1.0, 4.0], dtype=torch.float64, device=DEV)
    scratch = L.value_norm_scratch(n, DEV)
    odd = C.cast(C.c_void_p(block.data_ptr() + 4), L.c_f64_p)
    lib, f, d = L.lib, L.fptr, L.f64ptr
    calls = [(-2, lambda: lib.hgym_value_denormalize(0, f(x), f(dst), d(block), 1e-2, _stream())),
             (-2, lambda: lib.hgym_value_normalize(0, f(x), d(block), 1e-2, _stream())),
             (-2, lambda: lib.hgym_value_norm_merge(-1, f(x), d(block), d(scratch), _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, None, f(dst), d(block), 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, f(x), None, d(block), 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, f(x), f(dst), None, 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, f(x), f(dst), d(block), -1e-2, _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, f(x), f(dst), d(block), float("nan"), _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n, f(x), f(dst), odd, 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_denormalize(n - 8, f(x), f(x[4:]), d(block), 1e-2, _stream())),      # overlapping, not the same
             (-1, lambda: lib.hgym_value_normalize(n, None, d(block), 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_normalize(n, f(x), d(block), float("inf"), _stream())),
             (-1, lambda: lib.hgym_value_normalize(n, f(x), odd, 1e-2, _stream())),
             (-1, lambda: lib.hgym_value_norm_merge(n, None, d(block), d(scratch), _stream())),
             (-1, lambda: lib.hgym_value_norm_merge(n, f(x), None, d(scratch), _stream())),
             (-1, lambda: lib.hgym_value_norm_merge(n, f(x), d(block), None, _stream())),
             (-1, lambda: lib.hgym_value_norm_merge(n, f(x), odd, d(scratch), _stream())),
             (-1, lambda: lib.hgym_value_norm_merge(n, f(x), d(block), C.cast(C.c_void_p(scratch.data_ptr() + 4), L.c_f64_p), _stream()))]
    for i, (code, call) in enumerate(calls):
        assert call() == code, i
    torch.cuda.synchronize()
    assert bool((x == 3.0).all()) and bool((dst == 777.0).all()) and [float(v) for v in block.cpu()] == [5.0, 1.0, 4.0]
    assert not bool(scratch.any())


@pytest.mark.parametrize("n,skew", [(1, 0), (CH - 1, 4), (2 * CH + 1, 0), (2 * CH + 1, 12)])
def test_guard_bands(n, skew):
    """Every pointer carved at the header's size from a 0xFF arena: bands clean after every call, outputs equal to the unguarded twin's."""
    import hgym
    g = torch.Generator().manual_seed(n + skew)
    host = (1.0 + torch.randn(n, generator=g, dtype=torch.float64)).float()
    sizes = [4 * n, 4 * n, 8 * 3, 8 * V.scratch_doubles(n)]
    out = {}
    for kind, mem in (("guarded", GC.Arena(DEV, GC.arena_bytes(*sizes))), ("twin", GC.Plain(DEV))):
        x = mem.carve(n, torch.float32, skew=skew, name="x")
        x.copy_(host)
        dst = mem.carve(n, torch.float32, skew=skew, name="dst")
        block = mem.carve(3, torch.float64, name="block")
        block.copy_(torch.tensor(V.INITIAL, dtype=torch.float64))
        scratch = mem.zeros(V.scratch_doubles(n), torch.float64, name="scratch")
        hgym.value_norm_merge(x, block, scratch)
        mem.verify("hgym_value_norm_merge n=%d" % n)
        hgym.value_norm_merge(x, block, scratch)
        mem.verify("hgym_value_norm_merge (second call) n=%d" % n)
        hgym.value_denormalize(x, block, V.EPS, out=dst)
        mem.verify("hgym_value_denormalize n=%d" % n)
        hgym.value_normalize(x, block, V.EPS)
        mem.verify("hgym_value_normalize n=%d" % n)
        out[kind] = [t.clone() for t in (x, dst, block, scratch)]
        assert all(bool(torch.isfinite(t).all()) for t in out[kind])      # no guard byte was read and used
    for a, b in zip(out["guarded"], out["twin"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
