"""The CPU reference of the map-validated reduction (tests/policy_map_ref.py) on the three oracle-trained demo rule bases, with the
points of the greedy episode from the default start: the properties the criterion promises, checked on the oracle alone."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import policy_map_ref as ref
from tests.test_hip_reduce_batch import Trained

ENVS = ["mountaincar", "acrobot", "cartpole"]


@functools.lru_cache(maxsize=None)
def demo(env):
    """(Trained, tables, action VE values, the de-duplicated points of the default-start episode)"""
    probe = ob.Frirl(env, trig_mode=1)
    start = np.array([probe.dim(k)["values_def"] for k in range(probe.nstates)])
    t = Trained(env, start)
    f = t.fr.five
    pts = ref.dedup(ref.episode_points(t.fr, start))
    return t, np.array(f.u), np.array(f.ve), np.array(t.fr.action_vevalues), pts


@functools.lru_cache(maxsize=None)
def reduced(env, strategy):
    t, u, ve, ave, pts = demo(env)
    diag = ref.Diag()
    return ref.reduce_map(u, ve, t.rant, t.rconc, pts, ave, strategy, diag=diag), diag


def test_episode_points_are_the_oracles_episode():
    """the roll-out helper visits what orc_episode_eval visits: same number of steps; few distinct points"""
    for env, steps, distinct in (("mountaincar", 472, 36), ("acrobot", 57, 36), ("cartpole", 1000, 5)):
        t, _, _, _, pts = demo(env)
        t.restore(t.rant, t.rconc)
        assert len(ref.episode_points(t.fr, t.start)) == steps + 1 == t.baseline()[0] + 1
        assert len(pts) == distinct


@pytest.mark.parametrize("strategy", [1, 2])
@pytest.mark.parametrize("env", ENVS)
def test_reduced_rule_base_keeps_the_map(env, strategy):
    t, u, ve, ave, pts = demo(env)
    out, diag = reduced(env, strategy)
    kept = out.kept
    assert kept == sorted(set(kept)) and set(kept) <= set(range(t.R0)) and 1 <= len(kept) < t.R0, "increasing, a subset, something removed"
    assert out.tries <= t.R0 and diag.evaluations >= len(pts) * 2
    best0, _ = ref.policy_map(ref.make_five(u, ve, t.rant, t.rconc), pts, ave)
    best1, _ = ref.policy_map(ref.make_five(u, ve, t.rant[kept], t.rconc[kept]), pts, ave)
    assert (best0 == out.best0).all() and (best1 == best0).all()
    # the greedy episode on the reduced rule base is the un-reduced one's, observation by observation
    before = ref.episode_points(t.fr, t.start)
    t.restore(t.rant[kept], t.rconc[kept])
    after = ref.episode_points(t.fr, t.start)
    t.restore(t.rant, t.rconc)
    assert before.shape == after.shape and (before == after).all()


def test_untouched_cases():
    t, u, ve, ave, pts = demo("mountaincar")
    none = ref.reduce_map(u, ve, t.rant, t.rconc, pts[:0], ave, 1)
    assert none.kept == list(range(t.R0)) and none.tries == 0
    one = ref.reduce_map(u, ve, t.rant[:1], t.rconc[:1], pts, ave, 1)
    assert one.kept == [0] and one.tries == 0


def test_last_rule_survives():
    """A = 1: the map is 0 everywhere whatever the rules, so every removal is accepted -- down to one rule, which is never tried"""
    t, u, ve, ave, pts = demo("mountaincar")
    for strategy in (1, 2):
        out = ref.reduce_map(u, ve, t.rant, t.rconc, pts, ave[:1], strategy)
        order = ref.candidate_order(t.rconc, strategy)
        assert out.kept == [order[-1]] and out.tries == t.R0 - 1


def test_candidate_order_is_stable():
    q = np.array([0.5, -0.5, 0.0, 2.0, -2.0, 0.0])
    assert ref.candidate_order(q, 1) == [2, 5, 0, 1, 3, 4] and ref.candidate_order(q, 2) == [3, 4, 0, 1, 2, 5]


def test_log_points_order_and_dedup():
    """one agent, two logs, T = 5: start records give obs, the others q_obs; first occurrence over (log, record); bit-wise"""
    obs = np.arange(20, dtype=np.float64).reshape(2, 5, 2) + 100
    q = np.zeros((2, 5, 2))
    q[0, 1], q[0, 2], q[0, 4] = (1, 1), (2, 2), (1, 1)
    q[1, 1], q[1, 2], q[1, 3] = (2, 2), (-0.0, 0.0), (0.0, 0.0)
    start = np.array([[1, 0, 0, 1, 0], [1, 0, 0, 0, 0]], dtype=np.uint8)
    success = np.array([[0, 0, 1, 0, 0], [0, 0, 0, 1, 0]], dtype=np.int32)
    length = np.array([5, 4], dtype=np.int32)
    pts, over = ref.log_points(obs, q, success, start, length, 1, 10)
    want = [obs[0, 0], (1, 1), (2, 2), obs[0, 3], obs[1, 0], (-0.0, 0.0), (0.0, 0.0)]
    assert over[0] == 0 and pts[0].tobytes() == np.array(want, dtype=np.float64).tobytes()
    ok, _ = ref.log_points(obs, q, success, start, length, 1, 10, only_successful=True)       # log 0's second episode fails
    want_ok = [obs[0, 0], (1, 1), (2, 2), obs[1, 0], (-0.0, 0.0), (0.0, 0.0)]
    assert ok[0].tobytes() == np.array(want_ok, dtype=np.float64).tobytes()
    cut, over = ref.log_points(obs, q, success, start, length, 1, 3)
    assert over[0] == 1 and cut[0].tobytes() == np.array(want[:3], dtype=np.float64).tobytes()
    two, _ = ref.log_points(obs, q, success, start, length, 2, 10)                            # the same logs as two agents' one log each
    assert len(two[0]) == 4 and len(two[1]) == 4 and two[1][1].tolist() == [2.0, 2.0]
