"""CPU side of the TD-target tests (no GPU): the restated construct loop of tests/target_ref.py is the oracle's loop under target SARSA,
and the cases are worth running under target Q -- every greedy pick keeps its margin, every exploring agent takes actions other than
the greedy one and ends with another rule base than under SARSA, and a greedy agent does not notice the target.
"""
import numpy as np
import pytest

from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests import target_ref as tr


def _oracle(r):
    """A chain of explore_rows_cases.chain with the last episode's steps and reward beside it, as target_ref.chain returns them."""
    return dict(r, ep_steps=r["fr"].ep_steps, ep_reward=r["fr"].ep_reward)


def _same_agent(a, b):
    """Two chains (target_ref.chain's dicts) bit for bit: verdict, episodes, steps, last episode, rule base, sticky flag."""
    assert (a["converged"], a["episodes"], a["total_steps"]) == (b["converged"], b["episodes"], b["total_steps"])
    assert (a["ep_steps"], xc.bits(a["ep_reward"])) == (b["ep_steps"], xc.bits(b["ep_reward"]))
    assert tr.rule_base(a["fr"]) == tr.rule_base(b["fr"])
    assert int(a["fr"].fus) == int(b["fr"].fus)


@pytest.mark.parametrize("env", tr.DEMOS)
def test_the_restated_loop_under_sarsa_is_the_oracles_chain(env):
    """Every agent of explore_rows_cases.CASES over target_ref.EPISODES episodes: rule count, antecedents, consequents, steps, episodes,
    verdict, the last episode's steps and reward bits and the sticky flag equal explore_rows_cases.chain's; so do the pick counters."""
    E, sets, seed, _ = xc.CASES[env]
    for e in range(E):
        eps, h = sets[e % len(sets)]
        ref = xc.chain(env, xc.ID_BASE + e, seed, tr.EPISODES[env] + 1, lambda k: xc.epsilon_at(eps, h, k))
        got = tr.agent_run(env, e, tr.SARSA)
        _same_agent(got, _oracle(ref))
        s, o = got["stats"], ref["stats"]
        assert (s["picks"], s["explored"], s["changed"]) == (o["picks"], o["explored"], o["changed"]), (e, s, o)
        assert xc.bits(s["min_gap"]) == xc.bits(o["min_gap"]) or (np.isnan(s["min_gap"]) and np.isnan(o["min_gap"])), (e, s, o)


@pytest.mark.parametrize("env", tr.DEMOS)
def test_cases_are_admitted_under_target_q(env):
    """Agents, sets, seed and ids of explore_rows_cases.CASES over 8 / 9 / 7 episodes under target Q.  Measured (min gap over the
    exploring agents; steps with g != a' per exploring agent):
      mountaincar  1.27e-6   74 .. 519
      acrobot      4.75e-6   10 .. 251
      cartpole     3.29e-6    7 .. 59
    and on the case crossed with hyper-parameter rows 1.06e-6, 11 .. 218."""
    E, sets, seed, _ = xc.CASES[env]
    runs = [tr.agent_run(env, e, tr.Q) for e in range(E)]
    exploring = [e for e in range(E) if sets[e % len(sets)][0] > 0]
    print(env, "min_gap %.3g" % min(runs[e]["stats"]["min_gap"] for e in exploring), "changed", [runs[e]["stats"]["changed"] for e in exploring],
          "steps", [r["total_steps"] for r in runs])
    for e, r in enumerate(runs):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, r["stats"])
        sarsa = tr.agent_run(env, e, tr.SARSA)
        assert sarsa["stats"]["min_gap"] >= hc.MIN_GAP, (e, sarsa["stats"])
        if e in exploring:
            assert r["stats"]["changed"] >= 5, (e, r["stats"])
            assert tr.rule_base(r["fr"]) != tr.rule_base(sarsa["fr"]), (e, "target Q ends where SARSA ends")
        else:                                              # a greedy agent: a' == g at every step
            assert r["stats"]["explored"] == 0
            _same_agent(r, sarsa)


def test_every_set_occurs_under_both_targets():
    for env in tr.DEMOS:
        col = tr.mixed_column(env)
        assert col.dtype == np.uint8 and len(col) == xc.CASES[env][0]


def test_the_case_crossed_with_hyper_parameter_rows_is_admitted():
    """explore_rows_cases' acrobot cross case with target e mod 2: margins kept, every exploring Q agent takes other actions."""
    col = tr.cross_column()
    runs = [tr.cross_run(e) for e in range(xc.CROSS_E)]
    print("cross min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs), [r["stats"]["changed"] for r in runs])
    for e, (r, (name, (eps, h))) in enumerate(zip(runs, xc.cross_sets())):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, name, r["stats"])
        if col[e] == tr.SARSA:
            _same_agent(r, _oracle(xc.cross_run(e)))
        elif eps > 0:
            assert r["stats"]["changed"] >= 5 and tr.rule_base(r["fr"]) != tr.rule_base(xc.cross_run(e)["fr"]), (e, name)
    assert any(col[e] == tr.Q and x[0] > 0 for e, (_, x) in enumerate(xc.cross_sets()))


@pytest.mark.parametrize("taught", [False, True], ids=["untaught", "taught"])
@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_point_cases_stay_under_the_near_tie_cap(nant, A, taught):
    """A dry run of the mirrors of the caller-stepped case (the reference alone; 16 agents, 5 episodes, epsilon 0.4 over horizon e mod 4,
    target (e // 4) mod 2, with and without a scripted teacher): near-ties are at most a tenth of the picks, at least 10 learning steps
    of the shape have g != a', and they occur under target Q."""
    env, starts, mirrors = tr.point_mirrors(nant, A, taught)
    for ep in range(1, xc.POINT_EPISODES + 1):
        for m in mirrors:
            if not m.converged:
                m.target_episode(env, None, ep)
    near, picks = sum(m.near for m in mirrors), sum(m.picks for m in mirrors)
    off = [m.off_policy for m in mirrors]
    print(nant, A, taught, "near", near, "picks", picks, "g != a'", off, "taught", sum(m.taught for m in mirrors))
    assert near * 10 <= picks, (near, picks)
    assert sum(off) >= 10
    assert sum(o for o, m in zip(off, mirrors) if m.target == tr.Q) >= 10
    assert taught == (sum(m.taught for m in mirrors) > 0)
