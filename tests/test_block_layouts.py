"""CPU-only: the slot names of the three device blocks every layer passes around -- HgymNet.opt_state (HGYM_OPT_*), HgymEnvOut.log_stats
(HGYM_LOG_*) and HgymEnvState.counters (HGYM_CNT_*) -- in hgym/_lib.py against the defines of include/hgym.h, and the two host decoders
hgym.opt_summary / hgym.log_stats_summary on hand-written blocks."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_NAMES = ["LR", "STEP", "KL_SUM", "SURROGATE_SUM", "VALUE_SUM", "ENTROPY_SUM", "GRAD_NORM", "MINIBATCHES", "KL_LAST", "GRAD_SQNORM", "AUX_SUM",
             "STEP_SIZE", "SQRT_BC2", "PROLOGUE_STEP", "BETA1_POW", "BETA2_POW"]
CNT_NAMES = ["STEP", "RESETS", "RING", "RESET_CALL"]
LOG_NAMES = ["TERMS", "STEPS", "CLEAR", "RING_HEAD", "RING_FILL", "RING", "RETURNS", "LENGTHS", "STATS"]
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53]


def _header_defines(prefix):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgym.h")).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"#define\s+HGYM_%s_([A-Z0-9_]+)\s+(\d+)\s*$" % prefix, hdr, flags=re.M)}


def test_opt_state_names_match_the_header():
    from hgym import _lib as L
    d = _header_defines("OPT")
    assert set(d) == set(OPT_NAMES) | {"STATE"}, set(d) ^ set(OPT_NAMES)
    for nm in OPT_NAMES + ["STATE"]:
        assert d[nm] == getattr(L, "OPT_" + nm), nm
    assert d["STATE"] == 16 and sorted(d[nm] for nm in OPT_NAMES) == list(range(16))          # every slot named exactly once


def test_counter_names_match_the_header():
    from hgym import _lib as L
    d = _header_defines("CNT")
    assert set(d) == set(CNT_NAMES), set(d) ^ set(CNT_NAMES)
    for nm in CNT_NAMES:
        assert d[nm] == getattr(L, "CNT_" + nm), nm
    assert sorted(d.values()) == list(range(4))


def test_log_stats_names_match_the_header_and_regions_do_not_overlap():
    from hgym import _lib as L
    d = _header_defines("LOG")
    assert set(d) == set(LOG_NAMES), set(d) ^ set(LOG_NAMES)
    for nm in LOG_NAMES:
        assert d[nm] == getattr(L, "LOG_" + nm), nm
    assert d["TERMS"] + 22 == d["STEPS"] and L.NUM_REWARDS == 22
    assert d["STEPS"] < d["CLEAR"] <= d["RING_HEAD"]
    assert d["RING_HEAD"] != d["RING_FILL"] and d["CLEAR"] <= d["RING_FILL"] < d["RETURNS"] and d["RING_HEAD"] < d["RETURNS"]
    assert d["RETURNS"] + d["RING"] == d["LENGTHS"]
    assert d["LENGTHS"] + d["RING"] <= d["STATS"]


@pytest.mark.parametrize("minibatches,aux", [(7, True), (0, True), (7, False)])
def test_opt_summary_reads_the_named_slots(minibatches, aux):
    from hgym import opt_summary, _lib as L
    o = [float(p) for p in PRIMES]              # a distinct prime in every slot: a wrong slot gives a wrong quotient
    o[L.OPT_MINIBATCHES] = float(minibatches)
    n = float(minibatches) if minibatches else 1.0
    got = opt_summary(o, aux)
    assert got == dict(mean_value_loss=11.0 / n, mean_surrogate_loss=7.0 / n, denoise_loss=(31.0 / n if aux else None), learning_rate=2.0)
    import torch
    assert opt_summary(torch.tensor(o, dtype=torch.float64), aux) == got


@pytest.mark.parametrize("fill,steps", [(0, 4), (3, 4), (100, 4), (3, 0)])
def test_log_stats_summary_slices_and_means(fill, steps):
    from hgym import log_stats_summary, _lib as L
    terms = ["t%02d" % k for k in range(L.NUM_REWARDS)]
    ls = [1000.0 + k for k in range(L.LOG_STATS)]               # every slot distinct
    ls[L.LOG_STEPS], ls[L.LOG_RING_FILL] = float(steps), float(fill)
    names = ["t21", "t00", "t07"]                                # a subset, in the caller's order
    ep, returns, lengths = log_stats_summary(ls, names, terms)
    div = float(steps) if steps else 1.0
    assert list(ep) == ["rew_t21", "rew_t00", "rew_t07"]
    assert ep == {"rew_t21": 1021.0 / div, "rew_t00": 1000.0 / div, "rew_t07": 1007.0 / div}
    assert returns == [1032.0 + k for k in range(fill)] and lengths == [1132.0 + k for k in range(fill)]
    import torch
    t = torch.tensor(ls, dtype=torch.float32)
    assert log_stats_summary(t, names, terms) == (ep, returns, lengths)
    assert t.tolist() == ls                                      # a pure read
