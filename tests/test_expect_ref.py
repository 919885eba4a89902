"""CPU side of the expected-SARSA tests (no GPU): the gamma-0 restatement of the update (tests/expect_ref.py) is the oracle's update where
the value is a conclusion, the weights of the expectation are the frequencies of the oracle's pick, and the cases are worth running --
every greedy pick keeps its margin, every exploring expected agent learns towards values that are no conclusion of the action taken and
ends on another rule base than under SARSA and under Q, and a greedy agent does not notice the flag.
"""
import math

import numpy as np
import pytest

from oracle import binding as ob
from tests import expect_ref as er
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests import target_ref as tr
from tests.test_target_ref import _same_agent


@pytest.mark.parametrize("env", er.DEMOS)
def test_the_value_loop_is_the_point_loop_where_the_value_is_a_conclusion(env):
    """With v = Q(s', a') and with v = Q(s', g) the loop of expect_ref.chain ends on target_ref.chain under SARSA and under Q, bit for
    bit, for every agent of explore_rows_cases.CASES (their own seeds)."""
    E, sets, seed, _ = xc.CASES[env]
    for e in range(E):
        for mode, target in ((er.SARSA, tr.SARSA), (er.Q, tr.Q)):
            got, ref = er.agent_run(env, e, mode, seed), tr.agent_run(env, e, target)
            _same_agent(got, ref)
            s, o = got["stats"], ref["stats"]
            assert (s["picks"], s["explored"], s["changed"]) == (o["picks"], o["explored"], o["changed"]), (e, s, o)


@pytest.mark.parametrize("A", [1, 2, 3, 21, 32])
def test_the_weights_are_the_frequencies_of_the_oracles_random_branch(A):
    """ob.e_greedy_pick at epsilon 1 always takes the random branch and chooses lround(u * A) clamped to A - 1: over 40 000 stream keys
    action 0 occurs with frequency 0.5 / A, action A - 1 with 1.5 / A and the others with 1 / A (A = 1: the one action always), each within
    five binomial standard deviations."""
    N = 40000
    counts = np.zeros(A, dtype=np.int64)
    for i in range(N):
        counts[ob.e_greedy_pick(0, A, 1.0, 0, 97, 5, 1 + i // 1000, i % 1000)] += 1
    w = np.full(A, 1.0 / A)
    if A > 1:
        w[0], w[A - 1] = 0.5 / A, 1.5 / A
    assert abs(w.sum() - 1.0) < 1e-12
    for a in range(A):
        sd = math.sqrt(N * w[a] * (1.0 - w[a]))
        assert abs(counts[a] - N * w[a]) <= 5.0 * sd, (A, a, int(counts[a]), N * w[a], sd)
    # and the contract's M / A is that weighting of the conclusions
    c = np.random.default_rng(A).uniform(-3.0, 3.0, A)
    v = er.expected_value(c, int(np.argmax(c)), 0.25)
    assert abs(v - (0.75 * c.max() + 0.25 * float(w @ c))) <= 1e-12
    assert er.expected_value(c, 0, 0.0) == c[0]


@pytest.mark.parametrize("env", er.DEMOS)
def test_cases_are_admitted_under_the_mixed_column(env):
    """Agents, sets and ids of explore_rows_cases.CASES under expect_ref.SEEDS with expected[e] = (e // nsets) % 2, over 8 / 9 / 7 episodes.
    Every agent keeps hparams_cases.MIN_GAP at every pick that stayed greedy (smallest margins over ALL agents of the column, SARSA ones
    included: mountaincar 1.10e-6, acrobot 7.18e-6, cartpole 3.29e-6; over the expected agents alone 5.67e-6, 8.60e-5 and 3.29e-6 -- the figures of a run of this test, which prints them); every exploring expected agent has at least 5 learning steps whose value differs from
    Q(s', a') in bits and ends on another rule base than under SARSA and under Q; an epsilon 0 agent ends on its SARSA chain bit for bit."""
    E, sets, _, _ = xc.CASES[env]
    col = er.mixed_column(env)
    runs = [er.agent_run(env, e, er.mode_of(col[e])) for e in range(E)]
    print(env, "min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs), "expected agents alone %.3g" % min(r["stats"]["min_gap"] for e, r in enumerate(runs) if col[e]),
          "value differs", [r["stats"]["value_differs"] for r in runs],
          "steps", [r["total_steps"] for r in runs])
    told_apart = 0
    for e, r in enumerate(runs):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, r["stats"])
        if not col[e]:
            continue
        sarsa = er.agent_run(env, e, er.SARSA)
        if er.agent_set(env, e)[0] > 0:
            assert r["stats"]["value_differs"] >= 5, (e, r["stats"])
            assert tr.rule_base(r["fr"]) != tr.rule_base(sarsa["fr"]), (e, "expected SARSA ends where SARSA ends")
            assert tr.rule_base(r["fr"]) != tr.rule_base(er.agent_run(env, e, er.Q)["fr"]), (e, "expected SARSA ends where Q ends")
            told_apart += 1
        else:
            assert r["stats"]["explored"] == 0 and r["stats"]["value_differs"] == 0
            _same_agent(r, sarsa)
    assert told_apart >= len(sets) - 1


def test_mountaincar_value_differs_at_every_step_of_the_annealed_episodes():
    """On mountaincar an exploring expected agent's value differs from Q(s', a') in bits at every learning step of the episodes inside
    its horizon (epsilon != 0 there) but the very first, where every consequent is still 0 and so is every value: counted per agent
    against the steps of those episodes."""
    env = "mountaincar"
    E, sets, _, _ = xc.CASES[env]
    col = er.mixed_column(env)
    for e in range(E):
        eps, h = er.agent_set(env, e)
        if not col[e] or eps == 0.0:
            continue
        r = er.chain(env, xc.ID_BASE + e, er.SEEDS[env], h + 1, lambda k: xc.epsilon_at(eps, h, k), er.EXPECTED)
        assert r["episodes"] == h and r["stats"]["value_differs"] == r["total_steps"] - 1, (e, r["stats"], r["total_steps"])


def test_the_case_crossed_with_hyper_parameter_rows():
    """explore_rows_cases' acrobot cross case with flag e mod 2.  An agent whose expected chain falls below MIN_GAP is left on SARSA
    (expect_ref.cross_column; MIN_GAP is not loosened).  The agents left on SARSA are pinned: expect_ref.CROSS_LEFT_ON_SARSA, none, so the
    column tests/test_hip_expect.py runs is e mod 2 (smallest gap 1.06e-6).  Every agent of the column keeps MIN_GAP."""
    col, want = er.cross_column(), er.cross_wanted()
    runs = [er.cross_run(e, er.mode_of(col[e])) for e in range(xc.CROSS_E)]
    print("cross column", col.tolist(), "left on SARSA", [e for e in range(xc.CROSS_E) if want[e] and not col[e]],
          "min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs))
    assert tuple(e for e in range(xc.CROSS_E) if want[e] and not col[e]) == er.CROSS_LEFT_ON_SARSA
    assert col.tolist() == [0 if e in er.CROSS_LEFT_ON_SARSA else e % 2 for e in range(xc.CROSS_E)]
    for e, r in enumerate(runs):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, r["stats"])
    assert any(col[e] and x[0] > 0 for e, (_, x) in enumerate(xc.cross_sets()))


@pytest.mark.parametrize("taught", [False, True], ids=["untaught", "taught"])
@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_point_cases_stay_under_the_near_tie_cap(nant, A, taught):
    """A dry run of the mirrors of the caller-stepped case (the reference alone; 16 agents, 5 episodes, epsilon 0.4 over horizon e mod 4,
    flag (e // 4) mod 2, with and without a scripted teacher): near-ties are at most a tenth of the picks, as tests/test_target_ref.py
    caps them, and the flagged agents have at least 10 learning steps whose value is not Q(s', a')."""
    env, starts, mirrors = er.point_mirrors(nant, A, taught)
    for ep in range(1, xc.POINT_EPISODES + 1):
        for m in mirrors:
            if not m.converged:
                m.target_episode(env, None, ep)
    near, picks = sum(m.near for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, taught, "near", near, "picks", picks, "value differs", [m.value_differs for m in mirrors], "taught", sum(m.taught for m in mirrors))
    assert near * 10 <= picks, (near, picks)
    assert sum(m.value_differs for m in mirrors if m.expected) >= 10
    assert all(m.value_differs == 0 for m in mirrors if not m.expected)
    assert taught == (sum(m.taught for m in mirrors) > 0)
