"""CPU side of the per-agent hyper-parameter tests (no GPU): the mixed batches of tests/test_hip_hparam_rows.py are worth running.
On the oracle alone: every set of a demo's mixed batch keeps the margin of the greedy picks, and the sets end after pairwise
different numbers of steps, so that a kernel that gives an agent another agent's row cannot pass; the caller-stepped mixed cases
stay under the near-tie cap under which picks may follow the device.
"""
import itertools

import numpy as np
import pytest

from tests import hparam_rows_cases as rc
from tests import hparams_cases as hc


@pytest.mark.parametrize("env,nsets", [("mountaincar", 3), ("acrobot", 6), ("cartpole", 6)])
def test_mixed_demo_batches_tell_the_sets_apart(env, nsets):
    """Per demo the default set plus its admitted trajectory sets (hc.TRAJ_CASES).  Measured (portable trig, maxR 512, 14 / 8 / 6
    episodes), total steps per set and the smallest margin of a demo's sets:
      mountaincar  10 022 / 9 720 / 8 568                       2.5e-6
      acrobot      1 106 / 1 539 / 1 186 / 947 / 2 763 / 741    1.06e-6
      cartpole     380 / 700 / 103 / 89 / 108 / 180             3.3e-6"""
    sets = rc.demo_sets(env)
    assert len(sets) == nsets and sets[0] == "default"
    runs = [hc.traj_run(env, name) for name in sets]
    print(env, [r["total_steps"] for r in runs], "min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs))
    for name, r in zip(sets, runs):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (name, r["stats"])
    for (na, a), (nb, b) in itertools.combinations(zip(sets, runs), 2):
        assert a["total_steps"] != b["total_steps"], (na, nb, a["total_steps"])


def test_columns_carry_each_agents_own_values():
    descs = [hc.point_desc(4, 5, name) for name in rc.point_sets(4, 5)]
    col = rc.columns(descs)
    assert set(col) == set(rc.COLUMN.values()) and all(len(v) == rc.POINT_E for v in col.values())
    assert col["skip_rules"].dtype == np.int32 and col["alpha"].dtype == np.float64
    for e, d in enumerate(descs):
        assert [col[rc.COLUMN[k]][e] for k in hc.HP_KEYS] == [d[k] for k in hc.HP_KEYS]
    assert sorted(set(rc.point_sets(4, 5))) == sorted(hc.SETS)          # 16 agents: every set twice
    for k in hc.HP_KEYS:                                                # every column differs between agents
        assert len(set(col[rc.COLUMN[k]].tolist())) > 1, k


@pytest.mark.parametrize("nant,A", rc.POINT_SHAPES)
def test_point_cases_stay_under_the_near_tie_cap(nant, A):
    """A dry run of the mirrors of the mixed caller-stepped case (the oracle alone, 16 agents, 4 episodes, agent e under set
    (e + ROTATE) mod 8): picks at which the oracle's two best conclusions lie within 1e-12 relative are at most a tenth of the picks,
    the cap on picks that may follow the device.  Agents under different sets end with different rule bases.
    Measured near-ties / picks at rotation 0: 2 x 3 50 / 1044, 4 x 5 45 / 2348, 5 x 11 36 / 2514, 8 x 3 40 / 2494 (at most 4.8 %):
    no shape needs another rotation."""
    d, env, starts, descs, mirrors = rc.point_case(nant, A)
    for _ in range(rc.POINT_EPISODES):
        for m in mirrors:
            if not m.converged:
                m.episode(env, None)
    near, picks = sum(m.near for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, "rotation", rc.ROTATE[(nant, A)], "near", near, "picks", picks, "rules", [m.five.R for m in mirrors])
    assert near * 10 <= picks, (near, picks)
    never = [m for m, name in zip(mirrors, rc.point_sets(nant, A)) if name == "never_insert"]
    assert never and all(m.five.R == 2 ** nant for m in never)
    assert any(m.five.R > 2 ** nant for m in mirrors)
