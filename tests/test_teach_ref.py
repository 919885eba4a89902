"""The reference of the imitation tests alone (tests/teach_ref.py), on the CPU: the logs the GPU tests replay hold what those tests
need -- every kind of episode end, every branch of the update, a refused append at a small capacity -- and the scripted teachers do
what they are for."""
import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import teach_ref as tr

POINT_SHAPES = [(2, 3), (2, 11), (4, 3), (4, 11), (6, 3), (6, 11), (8, 3), (8, 11), (3, 32)]
DEMOS = ["mountaincar", "acrobot", "cartpole"]


def cases():
    return [("point", s) for s in POINT_SHAPES] + [("demo", env) for env in DEMOS]


def load(kind, what):
    return tr.point_case(*what) if kind == "point" else tr.demo_case(what)


@pytest.mark.parametrize("kind,what", cases())
def test_every_log_holds_every_kind_of_episode(kind, what):
    d, log = load(kind, what)
    assert log["obs"].shape[1] <= 200 and d["max_steps"] <= 120
    for e, ends in enumerate(log["ends"]):
        kinds = [k for k, _ in ends]
        assert "success" in kinds and "cut" in kinds and "max_steps" in kinds, (what, e, ends)
        assert all(0 <= a < d["A"] for a in log["action"][e, : log["length"][e]])
        assert log["start"][e, 0] == 1 and int(log["start"][e].sum()) == len(ends)


@pytest.mark.parametrize("kind,what", cases())
def test_every_log_takes_every_branch_of_the_update(kind, what):
    d, log = load(kind, what)
    mirrors = tr.mirrors_for(d, log, 512)
    for e, m in enumerate(mirrors):
        assert m.replay(log, e) == int(log["length"][e])
        b = m.branches
        assert b[tr.INSERTED] > 0 and b[tr.EXACT] > 0 and b[tr.SPREAD] > 0 and b[tr.FULL] == 0, (what, e, b)
        assert m.skipped >= 3 and m.refused == 0 and m.episode_no == len(log["ends"][e])
        assert m.five.R == 2 ** d["nant"] + b[tr.INSERTED]
    assert sum(m.same_point for m in mirrors) > 0, "no record repeats state cell and action: the one-conclusion form would go untested"


@pytest.mark.parametrize("kind,what", [("point", (4, 3)), ("point", (6, 11)), ("demo", "cartpole")])
def test_small_capacity_refuses_appends(kind, what):
    d, log = load(kind, what)
    maxR = 2 ** d["nant"] + 8
    mirrors = tr.mirrors_for(d, log, maxR)
    for e, m in enumerate(mirrors):
        m.replay(log, e)
        assert m.five.R <= maxR and (m.refused == 1) == (m.branches[tr.FULL] > 0)
    assert sum(m.refused for m in mirrors) > 0 and any(m.five.R == maxR for m in mirrors)


def test_second_pass_starts_again_at_record_zero():
    d, log = tr.point_case(4, 3)
    one, two = tr.mirrors_for(d, log, 512)[0], tr.mirrors_for(d, log, 512)[0]
    assert one.replay(log, 0) + one.replay(log, 0) == two.replay(log, 0, passes=2)
    assert one.trace == two.trace and one.episode_no == two.episode_no == 2 * len(log["ends"][0])
    assert (np.array(one.five.rconc[: one.five.R]) == np.array(two.five.rconc[: two.five.R])).all()


def test_out_of_range_action_ends_the_replay_before_it():
    d, log = tr.point_case(4, 3)
    bad = dict(log, action=log["action"].copy())
    bad["action"][0, 17] = d["A"]
    m = tr.mirrors_for(d, bad, 512)[0]
    assert m.replay(bad, 0, passes=2) == 17 and len(m.trace) == 17


class OracleEnv:
    """A demo's environment of the oracle behind PointEnv's step interface, remembering the state it returned last."""

    def __init__(self, env, start):
        self.fr, self.last = ob.Frirl(env), np.array(start, dtype=np.float64)

    def step(self, xp, x, a):
        ns, r, ok, _ = self.fr.env_step(float(a[0]), x[0])
        self.last = ns
        return ns[None], np.array([r]), np.array([ok])


def test_mountaincar_teacher_reaches_the_goal_in_its_first_episode():
    """Bang-bang on the sign of the velocity from the demo's own start state: the untaught first episode runs to max_steps, the
    taught one ends by success in under 200 steps and appends rules on the way."""
    d = frirl_amd.demo_describe("mountaincar")
    start = np.array(d["values_def"][: d["nstates"]])
    env = OracleEnv("mountaincar", start)
    law = tr.demo_teacher("mountaincar", d["A"])
    m = tr.TaughtMirror(d, start, 1024, teacher=lambda step: law(env.last, step))
    actions, steps, total = m.episode(env, None)
    assert steps < 200 and total == 1000.0 - 10.0 * (steps - 1), (steps, total)
    assert m.taught == steps + 1 and set(actions) <= {0, 2} and m.five.R > 2 ** d["nant"]
    env2 = OracleEnv("mountaincar", start)
    untaught = tr.TaughtMirror(dict(d, max_steps=300), start, 1024)
    assert untaught.episode(env2, None)[1] == 300


def test_a_teacher_that_names_no_action_leaves_the_pick_to_the_agent():
    d, _ = tr.point_case(4, 3)
    env, start = tr.PointEnv(3), np.array([0.3, -0.2, 0.5])
    plain = tr.Mirror(d, start, 512)
    taught = tr.TaughtMirror(d, start, 512, teacher=lambda step: 32)       # the reference's key 32
    assert plain.episode(env, None) == taught.episode(env, None) and taught.taught == 0
