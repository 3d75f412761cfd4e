"""CPU-only: the case list and the inputs of tests/test_fused_batch_edges_gpu.py, checked before anything runs on a GPU.

1. The constants of fused_batch_common.plan() are the ones csrc/hgym_net.hip and csrc/hgym_fused.hpp define (read from the defining
   lines); plan() reproduces the figures worked out by hand from the kernels.
2. BATCHES reaches every class of the batch plan: ragged tiles, empty / negative / partial splits, every tail of the unrolled pipeline,
   the summation chains on both sides of each loop switch, one-row and full tails.
3. The index lists and the spotlit rows are what make_case promises.
4. Every case's spot carries at least ten bars of every parameter tensor but std (float64 oracle alone), and the GPU test's metric,
   fed the oracle gradient with the spot removed in place of a kernel's result, exceeds the bar on every one of them."""
import pytest
import torch

import fused_batch_common as FB

PLANS = {B: FB.plan(B) for B in FB.BATCHES}


# ------------------------------------------------------------------------------------------------ 1. constants and plan
def test_constants_are_the_ones_the_sources_define():
    got = FB.source_constants()
    for name, (fn, _, pinned) in FB.SOURCE_LINES.items():
        assert got[name] == pinned, FB.RE_DERIVE % ("%s in %s: %s, pinned %s" % (name, fn, got[name], pinned))
    assert got["tile_rows"] == (FB.TILE, FB.TILE) and got["pad_rows"] == (FB.TILE,)
    assert got["step_rows"] == got["step_rows_idx"] == (FB.STEP,)
    assert got["dw_splits"] == (FB.SPLITS,)
    assert got["unroll"] == (FB.UNROLL - 1, FB.UNROLL, FB.UNROLL) and got["unroll_loop"] == (FB.UNROLL,)
    assert got["chains"] == got["chain_rest"] == (FB.CHAINS,) and got["chain_body"] == (FB.CHAIN_BODY, FB.CHAIN_BODY + FB.CHAINS)


def test_a_changed_constant_is_reported(monkeypatch):
    line = dict(FB.SOURCE_LINES)
    line["dw_splits"] = ("hgym_net.hip", r"w->dw_splits = (\d+);", (16,))
    monkeypatch.setattr(FB, "SOURCE_LINES", line)
    with pytest.raises(AssertionError, match="re-derive"):
        test_constants_are_the_ones_the_sources_define()
    line["dw_splits"] = ("hgym_net.hip", r"w->dw_splits = (\d+) \+ 0;", (8,))        # the defining line is gone
    with pytest.raises(AssertionError, match="re-derive"):
        FB.source_constants()


def test_plan_reproduces_the_figures_read_off_the_kernels():
    p = FB.plan(577)
    assert (p["tiles"], p["steps_total"], p["steps_per_split"]) == (10, 20, 3) and p["nsteps"] == [3, 3, 3, 3, 3, 3, 2, -1]
    assert p["np"] == [6, 6, 6, 6, 6, 6, 6, 0] and p["tail_rows"] == 1 and p["last_step"] == 18 and p["last_split"] == 6
    p = FB.plan(3073)
    assert (p["tiles"], p["steps_total"], p["steps_per_split"]) == (49, 98, 13) and p["nsteps"] == [13] * 7 + [7]
    assert p["np"] == [18] * 7 + [12] and p["split_rows"] == [416] * 7 + [161]
    for B in (1, 32, 33, 64):
        p = FB.plan(B)
        assert p["nsteps"] == [1, 1, 0, -1, -2, -3, -4, -5] and p["np"] == [6, 6, 0, 0, 0, 0, 0, 0] and p["used_splits"] == 2
        assert p["padding_steps"] == (1 if B <= 32 else 0) and p["split_rows"][:2] == [min(B, 32), max(B - 32, 0)]
    assert FB.plan(700)["nsteps"] == [3] * 7 + [1]
    assert FB.plan(61440)["nsteps"] == [240] * 8 and FB.plan(61440)["nblocks"] == 960
    # the chains: (passes of the 4-way body, passes of the remainder loop) of chain 0 and of chain 1
    assert [FB.chain_loops(n)[:2] for n in (1, 16, 17, 48, 49, 64, 65)] == [
        [(0, 1), (0, 0)], [(0, 1), (0, 1)], [(0, 2), (0, 1)], [(0, 3), (0, 3)], [(1, 0), (0, 3)], [(1, 0), (1, 0)], [(1, 1), (1, 0)]]


# ------------------------------------------------------------------------------------------------ 2. the case list
def _some(pred):
    return [B for B, p in PLANS.items() if pred(p)]


def test_batches_reach_every_class_of_the_plan():
    used_last = lambda p: p["nsteps"][p["used_splits"] - 1]
    partial = lambda p: used_last(p) < p["steps_per_split"]
    assert max(FB.BATCHES) == 4161 and FB.MAX_BATCH >= max(FB.BATCHES) and FB.MAX_BATCH % FB.TILE == 0
    assert set(FB.REDUCED) <= set(FB.BATCHES)
    # the first tile: a second step of nothing but padding; a ragged second step; exactly one tile
    assert len(_some(lambda p: p["B"] <= 32 and p["padding_steps"] == 1)) >= 3 and {1, 32} <= set(FB.BATCHES)
    assert len(_some(lambda p: 33 <= p["B"] <= 63)) >= 2 and 64 in FB.BATCHES
    # a one-row tail in a new tile
    assert {65, 129} <= set(_some(lambda p: p["tail_rows"] == 1 and p["B"] % FB.TILE == 1 and p["tiles"] > 1))
    # fewer used splits than 8, the others with nsteps <= 0 down to -5
    assert _some(lambda p: p["used_splits"] < FB.SPLITS and min(p["nsteps"]) == -(FB.UNROLL - 1))
    assert {n for p in PLANS.values() for n in p["nsteps"] if n <= 0} >= set(range(-5, 1))
    assert {p["used_splits"] for p in PLANS.values()} == {2, 4, 5, 6, 7, 8}        # (no B uses 1 or 3: 2 * tiles steps in eighths, rounded up)
    # all 8 used and full
    assert {449, 705} <= set(_some(lambda p: p["used_splits"] == FB.SPLITS and not partial(p)))
    # a partial last used split, fewer than 8 used / all 8 used
    assert {577, 800, 1025} <= set(_some(lambda p: p["used_splits"] < FB.SPLITS and partial(p)))
    assert {700, 1090, 1570, 3073} <= set(_some(lambda p: p["used_splits"] == FB.SPLITS and partial(p)))
    # a one-row tail behind full splits (the last used split full, its last step one valid row)
    assert _some(lambda p: p["tail_rows"] == 1 and not partial(p) and p["used_splits"] == FB.SPLITS and p["steps_per_split"] > 1)
    # every residue of nsteps mod 6 in a used split, and more than one revolution of the unrolled loop
    assert {n % FB.UNROLL for p in PLANS.values() for n in p["nsteps"] if n > 0} == set(range(FB.UNROLL))
    assert {n // FB.UNROLL for p in PLANS.values() for n in p["np"]} >= {0, 1, 2, 3}
    # a last used split whose steps differ from the others' by every count from 1 up
    assert {p["steps_per_split"] - used_last(p) for p in PLANS.values() if partial(p)} >= {1, 2, 6}
    # the summation chains: each tile count around a loop switch, and every (body, remainder) state
    assert {p["nblocks"] for p in PLANS.values()} >= {1, 2, 3, 16, 17, 48, 49, 50, 64, 65, 66}
    states = {c for p in PLANS.values() for c in p["chains"]}
    assert states >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)}
    mixed = _some(lambda p: len({c[0] for c in p["chains"]}) == 2)          # some chains in the 4-way body, others not
    assert {49, 50} <= {PLANS[B]["nblocks"] for B in mixed}
    # tails of 1 and of exactly 32 valid rows
    assert _some(lambda p: p["tail_rows"] == 1) and _some(lambda p: p["tail_rows"] == FB.STEP)
    assert {p["tail_rows"] for p in PLANS.values()} >= {1, 2, 15, 16, 17, 31, 32}


def test_spots():
    assert FB.spots_of(1) == ["tail"] and FB.spots_of(32) == ["tail", "row0"] and FB.spots_of(33) == ["tail", "row0"]
    assert FB.spots_of(577) == ["tail", "row0"]             # steps 18, 19 are split 6: its head is the tail's step
    assert FB.spots_of(3073) == ["tail", "split_head", "row0"]
    assert FB.spot_positions(3073, "split_head") == list(range(2912, 2944)) and FB.spot_positions(3073, "tail") == [3072]
    assert FB.spot_positions(700, "tail") == list(range(672, 700))
    assert {s for _, s in FB.CASES} == set(FB.SPOTS)
    assert all("tail" in FB.spots_of(B) and "row0" in FB.spots_of(B) for B in FB.BATCHES if B > 1)


# ------------------------------------------------------------------------------------------------ 3. index lists and spot rows
@pytest.mark.parametrize("B", [1, 2, 3, 33, 577])
def test_index_list(B):
    g = torch.Generator().manual_seed(B)
    S = B + 37
    idx = FB.make_index(B, S, g)
    assert idx.dtype == torch.int64 and idx.numel() == B and int(idx.min()) >= 0 and int(idx.max()) == S - 1
    vals, counts = torch.unique(idx, return_counts=True)
    if B >= 2:
        assert int(idx.min()) == 0
    assert sorted(counts.tolist()) == ([1] * (B - 2) + [2] if B >= 3 else [1] * B)


@pytest.mark.parametrize("B,spot", [(129, "tail"), (1090, "split_head"), (333, "row0")])
def test_spot_rows_are_unclipped_and_the_rest_is_not(B, spot):
    c = FB.make_case(B, spot, 7)
    cols, idx = c["cols"], c["idx"]
    dead = torch.ones(c["S"], dtype=torch.bool)
    dead[idx] = False
    assert int(dead.sum()) == c["S"] - len(set(idx.tolist())) and all(torch.isnan(t[dead]).all() for t in cols)
    assert all(torch.isfinite(t[idx]).all() for t in cols)
    want = FB.oracle_grad(c)
    sel = [t[idx].double() for t in cols]
    ratio = torch.exp(want["logp"] - sel[6])
    sp = torch.tensor(c["spot_pos"])
    rest = torch.ones(B, dtype=torch.bool)
    rest[sp] = False
    assert set(FB.spot_positions(B, spot)) <= set(c["spot_pos"])
    assert float((ratio[sp] - 1).abs().max()) < 1e-6                        # the bf16 error of the kernels' mu moves it by ~1e-2
    assert float((want["val"][sp] - sel[3][sp]).abs().max()) <= 0.2 / 4 + 1e-6
    assert float(sel[4][sp].abs().min()) >= c["factor"] and float((sel[5][sp] - want["val"][sp]).min()) >= c["factor"] * (1 - 1e-6)
    assert (ratio[rest] > 1.2).any() and (ratio[rest] < 0.8).any() and ((ratio[rest] > 0.8) & (ratio[rest] < 1.2)).any()
    assert ((want["val"] - sel[3])[rest].abs() > 0.2).any()


# ------------------------------------------------------------------------------------------------ 4. the condition on the inputs
def _shares(case, **kw):
    want = FB.oracle_grad(case, **kw)
    removed = FB.removed_spot(case, want, **kw)
    errs = FB.tensor_errors(removed, want["grads"].tensors())
    errs.pop("std")
    return errs


@pytest.mark.parametrize("B", FB.BATCHES)
def test_spot_carries_ten_bars_and_the_metric_sees_it_removed(B):
    bar = FB.bar_for(B)
    assert FB.BF16_OPERAND_TOL <= bar
    for spot in FB.spots_of(B):
        errs = _shares(FB.make_case(B, spot, 1000 + B))
        low = min(errs, key=errs.get)
        assert errs[low] >= FB.SHARE_FACTOR * bar, "B = %d, %s: %s carries %.3g < %g bars" % (B, spot, low, errs[low], FB.SHARE_FACTOR)
        # the metric on itself: a result that lacks the spot rows fails the GPU test's bar on every tensor
        assert all(e > bar for e in errs.values())


def test_bars_other_than_the_projects_sit_under_a_tenth_of_the_share():
    for B, bar in FB.BARS.items():
        assert B in FB.BATCHES and bar > FB.BF16_OPERAND_TOL
        for spot in FB.spots_of(B):
            assert bar <= min(_shares(FB.make_case(B, spot, 1000 + B)).values()) / FB.SHARE_FACTOR


@pytest.mark.parametrize("variant", ["g1", "a10", "tanh", "unclipped", "aux"])
def test_reduced_list_spots_carry_ten_bars(variant):
    """The tail spot of FB.REDUCED on the other kernels of the family, as tests/test_fused_batch_edges_gpu.py builds them."""
    for B in FB.REDUCED:
        case, kw, head = FB.variant_case(variant, B)
        errs = _shares(case, **kw)
        if head is not None:
            hidden, out, off, coef = head
            hp = FB.make_head(tuple(hidden), out)
            full, _ = FB.oracle_head_grad(case, hp, off, out, coef)
            alone, _ = FB.oracle_head_grad(case, hp, off, out, coef, case["spot_pos"])
            n = len(case["spot_pos"])
            for i, (f, a) in enumerate(zip(full, alone)):
                errs["denoiser.%d" % i] = FB.rel_l2(f - (n / B) * a, f)
        low = min(errs, key=errs.get)
        assert errs[low] >= FB.SHARE_FACTOR * FB.BF16_OPERAND_TOL, (variant, B, low, errs[low])
