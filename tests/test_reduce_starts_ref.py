"""The CPU model of the reduction against a set of start states (tests/reduce_starts_ref.py) against the oracle: with one start
state it is the reference's reduction (orc_reduce_run = frirl_sequential_run.c:170-350), its tree-walk form makes the decisions of
its sequential form, and a start that drop_bad_starts leaves out changes nothing else."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import reduce_starts_ref as ref
from tests.test_hip_reduce_batch import Trained, spread_starts


@functools.lru_cache(maxsize=None)
def default_agent(env):
    """the rule base the oracle learns from the default start state, and that start state (read before any replay moves it)"""
    probe = ob.Frirl(env, trig_mode=1)
    start = np.array([probe.dim(k)["values_def"] for k in range(probe.nstates)])
    return Trained(env, start), start


@pytest.mark.parametrize("env,strategy,want", [("mountaincar", 1, 28), ("mountaincar", 2, 52), ("acrobot", 1, 182), ("acrobot", 2, 155),
                                               ("cartpole", 1, 7)])
def test_one_start_is_the_reference_reduction(env, strategy, want):
    t, start = default_agent(env)
    got = ref.sequential(t, [start], strategy)
    want_rant, want_rconc = t.reduced(strategy)
    assert len(got.kept) == len(want_rconc) == want
    assert (t.rant[got.kept] == want_rant).all() and (t.rconc[got.kept] == want_rconc).all()
    steps, reward = t.baseline()
    assert got.per_start == [(1, steps, reward, reward)]             # tolerance 0: an accepted reward equals prev_reward


@functools.lru_cache(maxsize=None)
def mountaincar_starts(K, spread):
    t, start = default_agent("mountaincar")
    probe = ob.Frirl("mountaincar", trig_mode=1)
    s = spread_starts(probe, 16, spread)
    good = [k for k in range(16) if ref.Replayer(t).replay(list(range(t.R0)), s[k])[1] > t.fr.hparams["reward_good_above"]]
    return s[good[:K]]


@pytest.mark.parametrize("strategy,want", [(1, 30), (2, 52)])
def test_tree_walk_equals_sequential_for_three_starts(strategy, want):
    """mountaincar, K = 3 good starts at spread 0.3, depth 3 (the last round has 110 - 36 * 3 = 2 candidates)"""
    t, _ = default_agent("mountaincar")
    starts = mountaincar_starts(3, 0.3)
    seq = ref.sequential(t, starts, strategy)
    tree = ref.tree_walk(t, starts, strategy, 3)
    assert seq.kept == tree.kept and seq.per_start == tree.per_start
    assert len(seq.kept) == want
    # the oracle is shared with other tests: the model leaves it with the agent's own start state and the whole rule base
    assert [t.fr.dim(k)["values_def"] for k in range(t.fr.nstates)] == list(t.start)
    assert t.fr.five.R == t.R0 and (np.array(t.fr.five.rconc[: t.R0]) == t.rconc).all() and (np.array(t.fr.five.rant[: t.R0]) == t.rant).all()
    assert (tree.rounds, tree.rollouts) == ref.counters(t.R0, 3, 3, 3) == (37, 3 + 36 * 7 * 3 + 3 * 3)


def bad_start(t):
    """a start state from which the default mountaincar rule base does not reach the goal in time"""
    probe = ob.Frirl("mountaincar", trig_mode=1)
    rp = ref.Replayer(t)
    for s in spread_starts(probe, 200, 0.3, seed=5):                 # 2 of these 200 are not solved by the default rule base
        if not rp.replay(list(range(t.R0)), s)[1] > rp.good_above:
            return s
    raise AssertionError("no start state found whose baseline episode is not good")


def test_drop_bad_starts_equals_the_model_on_the_good_ones():
    t, _ = default_agent("mountaincar")
    good = mountaincar_starts(2, 0.3)
    bad = bad_start(t)
    starts = np.stack([good[0], bad, good[1]])
    dropped = ref.tree_walk(t, starts, 1, 3, drop_bad_starts=True)
    only_good = ref.tree_walk(t, good, 1, 3)
    assert dropped.kept == only_good.kept and dropped.used == [0, 2]
    assert [dropped.per_start[0], dropped.per_start[2]] == only_good.per_start
    used, steps, base, reward = dropped.per_start[1]
    assert used == 0 and steps > 0 and base == reward and not base > t.fr.hparams["reward_good_above"]
    assert (dropped.rounds, dropped.rollouts) == ref.counters(t.R0, 3, 3, 2)
    # literal: the bad start stays in and blocks every removal
    literal = ref.tree_walk(t, starts, 1, 3)
    assert literal.kept == list(range(t.R0)) and literal.used == [0, 1, 2] and literal.rounds == 37
    # only bad starts: finished after the baseline
    none = ref.tree_walk(t, np.stack([bad, bad]), 1, 3, drop_bad_starts=True)
    assert none.kept == list(range(t.R0)) and none.used == [] and (none.rounds, none.rollouts) == (0, 2)
    # start_count leaves the last start out
    two = ref.tree_walk(t, starts, 1, 3, count=2, drop_bad_starts=True)
    assert two.used == [0] and two.per_start[2] == (0, -1, 0.0, 0.0)
