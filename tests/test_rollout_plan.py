"""CPU: the fused rollout's launch plan (legged_robot.rollout_plan) against a restatement of the rules LeggedRobot.rollout_step and
the per-step PPO.fused_rollout_step reached through pointer identity before the plan existed, driven as OnPolicyRunner._rollout_fused and the
rollout tests of test_synth_path.py drove them (slots i, i + 1 and i + 2), over T, both modes, HGYM_ROWS_AHEAD, HGYM_L0_AHEAD and
HGYM_SHADOW; plus the facts of the protocol that the kernels rely on."""
import dataclasses
import itertools

import pytest

from humanoid.envs.base.legged_robot import rollout_plan

TS = (1, 2, 3, 24, 60)
CASES = list(itertools.product(TS, (False, True), (False, True), (False, True), (False, True)))
IDS = ["T%d-%s-rows%d-l0%d-shadow%d" % (T, "deferred" if d else "inline", r, l, s) for T, d, r, l, s in CASES]


def _today(T, deferred, rows_ahead, l0_ahead, shadows, slots):
    """The launches of the pointer-matching protocol for a storage of `slots` >= T slots, tensors as (name, slot) pairs and equality
    as data_ptr() identity: the caller's loop, the per-step PPO.fused_rollout_step, then LeggedRobot.rollout_step."""
    obs_all, priv_all = (lambda s: ("obs", s)), (lambda s: ("priv", s))
    obs_bf16, priv_bf16 = (lambda s: ("obs_bf16", s)), (lambda s: ("priv_bf16", s))
    ro_prev = ro_ahead = ro_l0 = None
    launches = []
    obs, priv = obs_all(0), priv_all(0)
    for i in range(T):
        s = i                                           # storage.step: the rollout starts on an empty storage
        next_obs, next_priv = obs_all(i + 1), priv_all(i + 1)
        ahead = (obs_all(i + 2), priv_all(i + 2)) if (i + 2 <= T and not deferred) else None
        own = obs == obs_all(s) and priv == priv_all(s)
        rec = dict(parity=(T - 1 - i) & 1, prev=ro_prev is not None, ahead=None, obs_older_ready=False, l0_ahead=None, l0_ready=None,
                   bf16_ahead=False)
        if deferred:
            sh = (obs_bf16(s), None) if (own and shadows) else None
            ro_ahead = ro_l0 = None
        else:
            sh = (obs_bf16(s), priv_bf16(s)) if (own and shadows) else None
            sh_next = obs_bf16(s + 1) if (sh is not None and s + 1 < slots and next_obs == obs_all(s + 1)) else None
            if not rows_ahead:
                ahead = None
            rec["obs_older_ready"] = ro_prev is not None and ro_ahead is not None and ro_ahead == (next_obs, next_priv)
            if ahead is not None:
                rec["ahead"] = ahead[0][1]
            ro_ahead = ahead
            if (ro_l0 is not None and rec["obs_older_ready"] and ro_l0[0] == obs
                    and ro_l0[2] == (None if sh is None else sh[0])):
                rec["l0_ready"] = ro_l0[1]
            ro_l0 = None
            if l0_ahead and ahead is not None and (sh is None) == (sh_next is None):
                rec["l0_ahead"] = i & 1
                rec["bf16_ahead"] = sh_next is not None
                ro_l0 = (next_obs, i & 1, sh_next)
        rec.update(shadow_obs=sh is not None and sh[0] is not None, shadow_priv=sh is not None and sh[1] is not None)
        ro_prev = True
        launches.append(rec)
        obs, priv = next_obs, next_priv
    return launches


@pytest.mark.parametrize("T, deferred, rows_ahead, l0_ahead, shadows", CASES, ids=IDS)
def test_plan_equals_the_pointer_matching_rules(T, deferred, rows_ahead, l0_ahead, shadows):
    plan = [dataclasses.asdict(p) for p in rollout_plan(T, deferred, rows_ahead, l0_ahead, shadows)]
    assert len(plan) == T
    # a storage longer than the rollout (test_synth_path.py: 24 of 60 slots) changes nothing
    for slots in (T, T + 36):
        assert plan == _today(T, deferred, rows_ahead, l0_ahead, shadows, slots), slots


@pytest.mark.parametrize("T, deferred, rows_ahead, l0_ahead, shadows", CASES, ids=IDS)
def test_plan_facts(T, deferred, rows_ahead, l0_ahead, shadows):
    plan = rollout_plan(T, deferred, rows_ahead, l0_ahead, shadows)
    first, last = plan[0], plan[-1]
    assert not first.prev and not first.obs_older_ready and first.l0_ready is None
    assert all(p.prev for p in plan[1:])
    assert last.ahead is None and last.l0_ahead is None and not last.bf16_ahead
    assert last.parity == 0 and all(a.parity != b.parity for a, b in zip(plan, plan[1:]))
    for i, p in enumerate(plan):
        if deferred:        # no critic tiles: none of their side jobs, and the priv shadow is left to deferred_values
            assert (p.ahead, p.obs_older_ready, p.l0_ahead, p.l0_ready, p.bf16_ahead, p.shadow_priv) == (None, False, None, None, False, False)
        assert p.l0_ready is None or p.obs_older_ready
        assert p.ahead in (None, i + 2) and (p.ahead is None or p.ahead <= T)
        assert p.l0_ahead in (None, i & 1) and p.l0_ready in (None, (i - 1) & 1)
        assert p.l0_ahead is None or p.ahead is not None
        assert p.bf16_ahead == (p.l0_ahead is not None and shadows)
        assert p.shadow_obs == shadows and p.shadow_priv == (shadows and not deferred)
        # what one launch leaves ahead is exactly what the next one takes as ready
        if i + 1 < T:
            assert plan[i + 1].obs_older_ready == (p.ahead == i + 2)
            assert plan[i + 1].l0_ready == (p.l0_ahead if plan[i + 1].obs_older_ready else None)


def test_steady_state_launches():
    """The default protocol at the runner's T: every launch but the first takes its older frames and first layer from the previous
    one, every launch but the last leaves them for the next."""
    plan = rollout_plan(60, False, True, True, True)
    assert all(p.obs_older_ready and p.l0_ready == (i - 1) & 1 for i, p in enumerate(plan) if i > 0)
    assert all(p.ahead == i + 2 and p.l0_ahead == i & 1 and p.bf16_ahead for i, p in enumerate(plan) if i < 59)
    assert not any(p.ahead or p.obs_older_ready or p.l0_ahead is not None for p in rollout_plan(60, False, False, True, True))
