"""CPU: PPO.exploration_noise -- the two filter constructors in float64, the fp32 twin of the table launch against
float64, config parsing with every ValueError, and hgym_policy_noise_table's argument checks (they return before anything touches a device)."""
import ctypes as C
import math

import pytest
import torch

from humanoid.algo.ppo import exploration_noise as EN

SIZES = (1, 2, 3, 60, 128)
U = 2.0 ** -24


def _toeplitz(r):
    t = torch.arange(r.numel())
    return r[(t[:, None] - t[None, :]).abs()]


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_colored_filter_is_the_cholesky_factor_of_its_toeplitz_covariance(T, beta):
    L, carry = EN.colored_filter(T, beta)
    assert carry is None and L.dtype == torch.float64 and L.shape == (T, T)
    assert torch.equal(L, torch.tril(L)) and bool((torch.diagonal(L) > 0).all())
    cov = _toeplitz(EN.colored_autocorrelation(T, beta))
    assert float((L @ L.T - cov).abs().max()) <= 1e-12
    assert float((torch.diagonal(L @ L.T) - 1.0).abs().max()) <= 1e-12 and abs(float(cov[0, 0]) - 1.0) <= 1e-15
    # the fp32 factor's rows still have unit norm to fp32 precision
    assert float(((L.float().double() ** 2).sum(1).sqrt() - 1.0).abs().max()) <= 2e-7


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("rho", [0.3, 0.9, 0.999])
def test_ar1_filter_and_carry_give_the_stationary_covariance(T, rho):
    L, c = EN.ar1_filter(T, rho)
    assert L.dtype == c.dtype == torch.float64 and L.shape == (T, T) and c.shape == (T,)
    assert torch.equal(L, torch.tril(L))
    t = torch.arange(T, dtype=torch.float64)
    want = torch.pow(torch.tensor(rho, dtype=torch.float64), (t[:, None] - t[None, :]).abs())
    cov = L @ L.T + c[:, None] * c[None, :]
    assert float((cov - want).abs().max()) <= 1e-12 and float((torch.diagonal(cov) - 1.0).abs().max()) <= 1e-12
    assert float((c - torch.tensor([rho ** (k + 1) for k in range(T)], dtype=torch.float64)).abs().max()) <= 1e-15


@pytest.mark.parametrize("kind,value", [("colored", 0.5), ("colored", 2.0), ("ar1", 0.9)])
def test_the_leading_rows_are_the_filter_of_a_shorter_rollout(kind, value):
    """A rollout of fewer steps than the storage holds uses the leading block of the storage's filter."""
    cfg = EN.parse_config({"kind": kind, EN.KINDS[kind][0]: value})
    big, cbig = EN.build_filter(cfg, 128)
    for T in (1, 2, 3, 24, 60):
        if kind == "ar1":      # the same closed form at every length
            small, csmall = EN.build_filter(cfg, T)
            assert torch.equal(big[:T, :T], small) and torch.equal(cbig[:T], csmall)
        else:                  # the Cholesky factor of the leading block of ONE Toeplitz matrix is the leading block of its factor
            r = EN.colored_autocorrelation(128, value)
            small = torch.linalg.cholesky(_toeplitz(r[:T]))
            assert float((big[:T, :T] - small).abs().max()) <= 1e-12


@pytest.mark.parametrize("T", SIZES)
def test_zero_is_the_exact_identity_without_a_carry(T):
    for cfg in ({"kind": "ar1", "rho": 0.0}, {"kind": "colored", "beta": 0}):
        c = EN.parse_config(cfg)
        L, carry = EN.build_filter(c, T)
        assert carry is None and torch.equal(L, torch.eye(T, dtype=torch.float64)) and EN.lag1(c, T) == 0.0
    # and the midpoint frequencies make beta = 0 white by themselves: r(k) = 0 for k >= 1
    r = EN.colored_autocorrelation(T, 0.0)
    assert abs(float(r[0]) - 1.0) <= 1e-15 and (T == 1 or float(r[1:].abs().max()) <= 1e-13)


def test_lag1_is_the_configured_correlation():
    assert EN.lag1(EN.parse_config({"kind": "ar1", "rho": 0.75}), 60) == 0.75
    r1 = EN.lag1(EN.parse_config({"kind": "colored", "beta": 0.5}), 60)
    L, _ = EN.colored_filter(60, 0.5)
    assert abs(r1 - float((L @ L.T)[5, 6])) <= 1e-12 and abs(r1 - 0.36) < 0.01      # 0.36: the figure the design note quotes


@pytest.mark.parametrize("T,tail", [(1, (1,)), (3, (5, 2)), (60, (7, 12)), (128, (3, 4))])
@pytest.mark.parametrize("kind,value", [("colored", 1.0), ("ar1", 0.9)])
def test_fp32_twin_against_float64(T, tail, kind, value):
    """The kernel's order of operations in fp32 against the same sums in float64 (on the fp32-rounded filter and draws): row t passes
    through at most t + 2 roundings -- one multiply, then up to t + 1 adds, the carry term one more -- each 2^-24 relative."""
    g = torch.Generator().manual_seed(T)
    filt, carry = EN.build_filter(EN.parse_config({"kind": kind, EN.KINDS[kind][0]: value}), T)
    filt = filt.float()
    carry = None if carry is None else carry.float()
    w = torch.randn(T, *tail, generator=g)
    state = torch.randn(*tail, generator=g) if carry is not None else None
    x32, _ = EN.table_reference(filt, carry, state, w, torch.float32)
    x64, b64 = EN.table_reference(filt, carry, state, w, torch.float64)
    assert x32.dtype == torch.float32 and x64.dtype == torch.float64
    steps = (torch.arange(T, dtype=torch.float64) + 2.0).view(T, *([1] * len(tail)))
    assert bool(((x32.double() - x64).abs() <= steps * U * b64).all())
    # and the float64 twin is the matrix product
    direct = torch.einsum("ts,s...->t...", torch.tril(filt.double()), w.double())
    if carry is not None:
        direct = direct + carry.double().view(T, *([1] * len(tail))) * state.double()
    assert float((x64 - direct).abs().max()) <= 1e-12
    # unit marginal variance by construction
    var = (torch.tril(filt.double()) ** 2).sum(1) + (0 if carry is None else carry.double() ** 2)
    assert float((var - 1.0).abs().max()) <= 1e-6


def test_config_parsing_and_every_refusal(monkeypatch):
    assert EN.parse_config(None) is None
    assert EN.parse_config({"kind": "ar1", "rho": 0.5}) == dict(kind="ar1", param="rho", value=0.5)
    assert EN.parse_config({"kind": "colored", "beta": 2}) == dict(kind="colored", param="beta", value=2.0)
    assert EN.parse_config({"kind": "colored", "beta": 0})["value"] == 0.0
    for bad, text in (({"kind": "ar1", "rho": 0.5, "gain": 1}, "unknown key 'gain'"), ({"kind": "colored", "rho": 0.5, "beta": 1}, "unknown key 'rho'"),
                      ({"kind": "pink", "beta": 1}, "kind='pink'"), ({"beta": 1}, "kind=None"), ({"kind": "ar1"}, "needs 'rho'"),
                      ({"kind": "ar1", "rho": 1.0}, "outside"), ({"kind": "ar1", "rho": -0.1}, "outside"),
                      ({"kind": "colored", "beta": 2.5}, "outside"), ({"kind": "colored", "beta": -1}, "outside"),
                      ({"kind": "colored", "beta": float("nan")}, "outside"), ({"kind": "ar1", "rho": "x"}, "not a number"),
                      ("colored", "a dict")):
        with pytest.raises(ValueError, match=text):
            EN.parse_config(bad)
    EN.check_setup(128, 12)
    with pytest.raises(ValueError, match="num_steps_per_env=129 exceeds the 128"):
        EN.check_setup(129, 12)
    with pytest.raises(ValueError, match="num_actions=13"):
        EN.check_setup(24, 13)
    # scripts/train.py's switches
    assert EN.config_from_env({}) is None
    assert EN.config_from_env({"HGYM_NOISE_COLOR": "0.5"}) == {"kind": "colored", "beta": 0.5}
    assert EN.config_from_env({"HGYM_NOISE_AR1": "0.9"}) == {"kind": "ar1", "rho": 0.9}
    with pytest.raises(ValueError, match="one filter at a time"):
        EN.config_from_env({"HGYM_NOISE_COLOR": "0.5", "HGYM_NOISE_AR1": "0.9"})
    # the train config's key is taken out of PPO.__init__'s keyword arguments
    from humanoid.algo.ppo import on_policy_runner as R
    from humanoid.algo import PPO
    kw, _ = R._split_algorithm_cfg({"clip_param": 0.2, R.NOISE_KEY: {"kind": "ar1", "rho": 0.9}})
    assert kw == {"clip_param": 0.2} and R.NOISE_KEY == "exploration_noise_cfg" and PPO.exploration_noise is None


def test_library_argument_checks():
    """Every refusal of hgym_policy_noise_table comes before anything is launched: it can be provoked without a device."""
    from hgym import _lib as L
    assert L.NOISE_MAX_STEPS == EN.MAX_STEPS == 128 and L.NUM_DOF == EN.MAX_ACTIONS
    buf = (C.c_float * 64)()
    step = (C.c_int64 * 1)()
    f, i = C.cast(buf, L.c_float_p), C.cast(step, L.c_i64_p)

    def call(T=2, n=1, A=12, filt=f, ld=4, carry=None, state=None, st=i, z=f):
        rc = L.lib.hgym_policy_noise_table(T, n, A, filt, ld, carry, state, 7, st, z, None)
        return rc, L.lib.hgym_last_error().decode()

    E_BADARG, E_SHAPE = -1, -2
    for kw, code, text in ((dict(T=0), E_SHAPE, "T=0"), (dict(T=129, ld=129), E_SHAPE, "T=129"), (dict(A=13), E_SHAPE, "A=13"),
                           (dict(A=0), E_SHAPE, "A=0"), (dict(n=0), E_SHAPE, "n=0"), (dict(ld=1), E_SHAPE, "ld_filt=1"),
                           (dict(filt=None), E_BADARG, "null"), (dict(st=None), E_BADARG, "null"), (dict(z=None), E_BADARG, "null"),
                           (dict(carry=f, state=None), E_BADARG, "state is NULL"),
                           (dict(z=C.cast(C.addressof(buf) + 2, L.c_float_p)), E_BADARG, "aligned")):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert math.isfinite(U)
