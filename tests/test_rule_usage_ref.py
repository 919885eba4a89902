"""The CPU reference of the rule usage, the stable order and the map-validated reduction under caller orders (tests/rule_usage_ref.py)
on the three oracle-trained demo rule bases with the points of the greedy episode from the default start: the properties the
statistic and the criterion promise, checked on the oracle alone."""
import functools

import numpy as np
import pytest

from tests import policy_map_ref as pm
from tests import rule_usage_ref as ref
from tests.test_policy_map_ref import ENVS, demo


@functools.lru_cache(maxsize=None)
def demo_usage(env):
    t, u, ve, ave, pts = demo(env)
    return ref.usage(pm.make_five(u, ve, t.rant, t.rconc), pts, ave)


def orders_of(env):
    """the candidate orders of tests/test_hip_reduce_orders.py for the demo rule base: reversed index, a fixed permutation, least-used first"""
    t = demo(env)[0]
    R = t.R0
    return {"reversed": list(range(R - 1, -1, -1)), "permutation": [int(r) for r in np.random.default_rng(5).permutation(R)],
            "usage": ref.stable_order(demo_usage(env)[0])}


@pytest.mark.parametrize("env", ENVS)
def test_usage_sums_to_the_point_count(env):
    t, u, ve, ave, pts = demo(env)
    total, peak, best = demo_usage(env)
    n = len(pts)
    assert total.shape == (t.R0,) and abs(total.sum() - n) <= 1e-12 * n, "every point hands out weights that sum to 1"
    assert (total >= 0).all() and (peak >= 0).all() and (peak <= 1).all() and (peak <= total).all()
    assert (best == pm.policy_map(pm.make_five(u, ve, t.rant, t.rconc), pts, ave)[0]).all()


def test_stable_order():
    for env in ENVS:
        q = demo(env)[0].rconc
        assert ref.stable_order(np.abs(q)) == pm.candidate_order(q, 1) and ref.stable_order(np.abs(q), True) == pm.candidate_order(q, 2)
    nan = float("nan")
    keys = np.array([0.5, nan, 0.0, 2.0, 0.5, nan, -1.0, 0.0])
    assert ref.stable_order(keys) == [6, 2, 7, 0, 4, 3, 1, 5] and ref.stable_order(keys, True) == [3, 0, 4, 2, 7, 6, 1, 5]
    assert ref.stable_order(np.array([0.0, -0.0, 0.0])) == [0, 1, 2] == ref.stable_order(np.array([0.0, -0.0, 0.0]), True)


@pytest.mark.parametrize("name", ["reversed", "permutation", "usage"])
@pytest.mark.parametrize("env", ENVS)
def test_reduction_under_any_order_keeps_the_map(env, name):
    t, u, ve, ave, pts = demo(env)
    order = orders_of(env)[name]
    out = ref.reduce_map_order(u, ve, t.rant, t.rconc, pts, ave, order)
    kept = out.kept
    assert kept == sorted(set(kept)) and set(kept) <= set(range(t.R0)) and 1 <= len(kept) < t.R0
    assert out.tries <= t.R0
    best0, _ = pm.policy_map(pm.make_five(u, ve, t.rant, t.rconc), pts, ave)
    best1, _ = pm.policy_map(pm.make_five(u, ve, t.rant[kept], t.rconc[kept]), pts, ave)
    assert (best0 == out.best0).all() and (best1 == best0).all()
    before = pm.episode_points(t.fr, t.start)
    t.restore(t.rant[kept], t.rconc[kept])
    after = pm.episode_points(t.fr, t.start)
    t.restore(t.rant, t.rconc)
    assert before.shape == after.shape and (before == after).all(), "the greedy episode is reproduced observation by observation"


def test_order_with_the_callers_strategy_order_is_the_strategy():
    t, u, ve, ave, pts = demo("mountaincar")
    for strategy in (1, 2):
        a = pm.reduce_map(u, ve, t.rant, t.rconc, pts, ave, strategy)
        b = ref.reduce_map_order(u, ve, t.rant, t.rconc, pts, ave, pm.candidate_order(t.rconc, strategy))
        assert a.kept == b.kept and a.tries == b.tries


def test_best_of_orders_picks_the_fewest_rules_and_the_lowest_k():
    t, u, ve, ave, pts = demo("mountaincar")
    o = orders_of("mountaincar")
    first = pm.candidate_order(t.rconc, 1)
    k, out, after = ref.reduce_map_orders(u, ve, t.rant, t.rconc, pts, ave, [first, o["usage"], first])
    assert after[0] == after[2] and after[k] == min(after) and k == after.index(min(after)) and len(out.kept) == after[k]
    k, out, after = ref.reduce_map_orders(u, ve, t.rant, t.rconc, pts[:0], ave, [first, o["usage"]])
    assert k == -1 and after == [t.R0, t.R0] and out.tries == 0
