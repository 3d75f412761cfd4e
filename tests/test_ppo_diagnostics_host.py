"""CPU-only: the host side of the diagnostics pass -- hgym.diag_from_block on hand-written sums, and the DIAG_* indices and the block size
of hgym/_lib.py against the defines of include/hgym.h."""
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgym.h")).read(), flags=re.S)
    return hdr, {k: int(v) for k, v in re.findall(r"#define\s+HGYM_DIAG_([A-Z_]+)\s+(\d+)", hdr)}


def test_diag_indices_and_block_size_match_the_header():
    from hgym import _lib as L
    hdr, d = _header_defines()
    names = ["COUNT", "KL", "APPROX_KL", "RATIO", "CLIPPED", "RATIO_MAX", "RATIO_MIN", "SURROGATE", "RET", "RET_SQ", "ERR_OLD", "ERR_OLD_SQ",
             "ERR_NEW", "ERR_NEW_SQ", "VALUE_CLIPPED", "ENTROPY"]
    assert set(d) == set(names) | {"SUMS", "ROWS_PER_PARTIAL", "MAX_ROWS"}, set(d) ^ set(names)
    for nm in names:
        assert d[nm] == getattr(L, "DIAG_" + nm), nm
    assert sorted(d[nm] for nm in names) == list(range(d["SUMS"]))           # every slot of the totals named once
    assert d["SUMS"] == L.DIAG_SUMS and d["ROWS_PER_PARTIAL"] == L.DIAG_ROWS_PER_PARTIAL == 256 and d["MAX_ROWS"] == 2 ** 31
    # the size macro, evaluated from the header's own text
    m = re.search(r"#define\s+HGYM_DIAG_BLOCK_DOUBLES\(total_rows\)\s*\\?\s*(.+)", hdr)
    expr = m.group(1).replace("(size_t)", "").replace("/", "//")
    for n in (0, 1, 255, 256, 257, 1000, 245760, 2 ** 31):
        want = eval(expr, {"total_rows": n, "HGYM_DIAG_SUMS": d["SUMS"], "HGYM_DIAG_ROWS_PER_PARTIAL": d["ROWS_PER_PARTIAL"]})
        assert L.diag_block_doubles(n) == want == 16 * (1 + (n + 255) // 256), n
    for name in ("hgym_ppo_diag_reset", "hgym_ppo_diag_reduce", "hgym_ppo_diagnostics"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)


def _block(**kw):
    from hgym import _lib as L
    b = [0.0] * L.DIAG_SUMS
    for k, v in kw.items():
        b[getattr(L, "DIAG_" + k)] = float(v)
    return b


def test_diag_from_block_on_hand_written_sums():
    from hgym import diag_from_block, DIAG_KEYS
    # 4 rows: R = 1, 2, 3, 6; V_old = R - (1, -1, 1, -1); V_new = R - (0.5, 0.5, 0.5, 0.5)
    R = [1.0, 2.0, 3.0, 6.0]
    eo, en = [1.0, -1.0, 1.0, -1.0], [0.5] * 4
    b = _block(COUNT=4, KL=0.08, APPROX_KL=0.04, RATIO=4.4, CLIPPED=1, RATIO_MAX=1.7, RATIO_MIN=0.6, SURROGATE=-2.0, RET=sum(R),
               RET_SQ=sum(r * r for r in R), ERR_OLD=sum(eo), ERR_OLD_SQ=sum(e * e for e in eo), ERR_NEW=sum(en),
               ERR_NEW_SQ=sum(e * e for e in en), VALUE_CLIPPED=2, ENTROPY=4 * 9.5)
    d = diag_from_block(b, 0.2)
    assert tuple(d) == DIAG_KEYS and all(isinstance(v, float) for k, v in d.items() if k != "samples")
    var_r = sum(r * r for r in R) / 4 - 3.0 ** 2           # 3.5
    exp = dict(samples=4, clip_fraction=0.25, kl=0.02, approx_kl=0.01, ratio_mean=1.1, ratio_max=1.7, ratio_min=0.6, surrogate=-0.5,
               entropy=9.5, value_clip_fraction=0.5, return_mean=3.0, return_std=math.sqrt(var_r), explained_variance=1.0 - 1.0 / var_r,
               explained_variance_new=1.0, value_rmse=1.0, value_rmse_new=0.5)
    assert d["samples"] == 4 and isinstance(d["samples"], int)
    for k, v in exp.items():
        assert d[k] == v or abs(d[k] - v) <= 1e-15 * abs(v), (k, d[k], v)
    # a torch tensor of a whole block (totals + partials) is accepted too
    import torch
    t = torch.tensor(b + [7.0] * 32, dtype=torch.float64)
    assert diag_from_block(t) == d


def test_explained_variance_exactly_zero_and_exactly_one():
    from hgym import diag_from_block
    R = [0.25, -1.5, 4.0, 2.0, 2.0]
    s1, s2 = sum(R), sum(r * r for r in R)
    # V_old = 0: the error IS the return -> 0 exactly; V_new = R: no error at all -> 1 exactly
    d = diag_from_block(_block(COUNT=5, RET=s1, RET_SQ=s2, ERR_OLD=s1, ERR_OLD_SQ=s2, ERR_NEW=0.0, ERR_NEW_SQ=0.0))
    assert d["explained_variance"] == 0.0 and d["explained_variance_new"] == 1.0
    assert d["value_rmse"] == math.sqrt(s2 / 5) and d["value_rmse_new"] == 0.0
    # a critic worse than the mean: negative
    d = diag_from_block(_block(COUNT=5, RET=s1, RET_SQ=s2, ERR_OLD=2 * s1, ERR_OLD_SQ=4 * s2, ERR_NEW=s1, ERR_NEW_SQ=s2))
    assert d["explained_variance"] == -3.0 and d["explained_variance_new"] == 0.0


def test_constant_returns_give_nan_and_no_samples_give_nan():
    from hgym import diag_from_block, DIAG_KEYS
    d = diag_from_block(_block(COUNT=3, RET=6.0, RET_SQ=12.0, ERR_OLD=0.3, ERR_OLD_SQ=0.05, ERR_NEW=0.0, ERR_NEW_SQ=0.0, RATIO=3.0,
                               RATIO_MAX=1.0, RATIO_MIN=1.0))
    assert d["return_std"] == 0.0 and math.isnan(d["explained_variance"]) and math.isnan(d["explained_variance_new"])
    assert d["ratio_mean"] == 1.0 and d["return_mean"] == 2.0 and d["value_rmse_new"] == 0.0
    # what the device leaves for M = 0: zero sums, max / min at their identities
    e = diag_from_block(_block(RATIO_MAX=-math.inf, RATIO_MIN=math.inf))
    assert tuple(e) == DIAG_KEYS and e["samples"] == 0
    assert all(math.isnan(v) for k, v in e.items() if k != "samples")
