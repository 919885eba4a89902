"""CPU side of the per-agent exploration tests (no GPU): the reference of tests/test_hip_explore_rows.py -- the oracle's construct
loop run one episode per call, each episode at the agent's own rate -- is the oracle's loop, and the cases are worth running: every
greedy pick keeps its margin, every exploring agent explores, every annealed agent runs past its horizon, and an agent that took its
neighbour's row would end elsewhere.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc


def _state(fr):
    R = fr.five.R
    return (R, fr.ep_steps, xc.bits(fr.ep_reward), fr.total_steps, np.array(fr.five.rant[:R]).tobytes(), np.array(fr.five.rconc[:R]).tobytes())


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("env", xc.DEMOS)
def test_a_chain_of_single_episodes_is_the_construct_loop(env, eps):
    """N - 1 calls of set_exploration(eps, 0, seed, id, episode=k - 1) + run(max_episodes=2) against one run(max_episodes=N): rule
    count, steps and reward bits of the last episode, total steps, antecedents and consequents bit for bit, and the same verdict."""
    _, _, seed, N = xc.CASES[env]
    whole = hc.demo_frirl(env, "default", trig_mode=1, maxR=xc.MAXR)
    whole.set_exploration(eps, 0, seed, xc.ID_BASE, episode=0)
    converged = int(whole.run(max_episodes=N))
    c = xc.chain(env, xc.ID_BASE, seed, N, lambda k: eps)
    assert c["converged"] == converged
    assert c["episodes"] == int(ob.lib().orc_frirl_episode_num(whole.h)) - (0 if converged else 1)
    assert _state(c["fr"]) == _state(whole)
    assert eps == 0.0 or c["stats"]["changed"] >= 5


def test_the_rate_falls_linearly_to_zero():
    assert [xc.epsilon_at(0.3, 4, k) for k in (1, 2, 3, 4, 5, 6)] == [0.3, 0.3 * 0.75, 0.3 * 0.5, 0.3 * 0.25, 0.0, 0.0]
    assert xc.epsilon_at(0.3, 0, 1) == xc.epsilon_at(0.3, 0, 10 ** 6) == 0.3
    assert xc.epsilon_at(0.1, 2, 2) == 0.1 * 0.5 and xc.epsilon_at(0.1, 3, 3) == 0.1 * (1.0 / 3.0)


@pytest.mark.parametrize("env", xc.DEMOS)
def test_cases_are_admitted(env):
    """Ids 77 + e, portable trig, maxR 512, agent e under set e mod nsets.  Measured:
      mountaincar  min gap 1.44e-6; converged 1,0,1,1,1,0,1,1,1; episodes 29,39,35,29,24,39,29,24,35; 149 172 steps; picks that changed
                   the action 0 / 86 .. 107 / 509 .. 523 per set; rules 90 .. 112
      acrobot      min gap 7.18e-6; none converges; 19 007 steps; changed 0 / 10 .. 13 / 55 .. 81 / 194 .. 221
      cartpole     min gap 3.29e-6; none converges; 4 897 steps; changed 0 / 7 .. 9 / 23 .. 38 / 59 .. 89"""
    E, sets, seed, N = xc.CASES[env]
    pairs = xc.agent_sets(env)
    runs = [xc.agent_run(env, e) for e in range(E)]
    print(env, "min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs), [r["converged"] for r in runs], [r["episodes"] for r in runs],
          sum(r["total_steps"] for r in runs), [r["stats"]["changed"] for r in runs])
    for e, (r, (eps, h)) in enumerate(zip(runs, pairs)):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, r["stats"])
        if eps > 0:
            assert r["stats"]["changed"] >= 5, (e, r["stats"])
        else:
            assert r["stats"]["explored"] == 0
        if h > 0:
            assert r["episodes"] > h, (e, r["episodes"], h)
        # under the neighbour's row at its own id the agent ends elsewhere: a row taken by launch slot is caught
        other = xc.agent_run(env, e, under=e + 1)
        assert (other["fr"].five.R, other["total_steps"]) != (r["fr"].five.R, r["total_steps"]), (e, r["total_steps"])
    m = xc.MEASURED[env]
    assert [r["converged"] for r in runs] == m["converged"] and [r["episodes"] for r in runs] == m["episodes"]
    assert sum(r["total_steps"] for r in runs) == m["total_steps"]
    if env == "mountaincar":
        assert sum(r["converged"] for r, (eps, h) in zip(runs, pairs) if h > 0) >= 4


def test_rows_crossed_with_hyper_parameter_rows_are_admitted():
    """Acrobot, 12 agents, 8 episodes, hyper-parameter set e mod 6 (the rows test's demo sets) crossed with exploration set e mod 4:
    every chain keeps the margin of its greedy picks, every exploring agent explores and runs past its horizon, all six and all four
    sets take part.  thr0 is paired with the greedy set alone: under (0.3, 4) its two best conclusions tie (1.2e-16 measured).
    Measured: min gap 1.06e-6; steps 1106 916 1186 928 2763 832 1347 882 1186 2759 1114 881; picks that changed the action 0 or 11 .. 182."""
    pairs = xc.cross_sets()
    assert len({name for name, _ in pairs}) == 6 and len({x for _, x in pairs}) == 4
    assert all(x == (0.0, 0) for name, x in pairs if name == "thr0")
    runs = [xc.cross_run(e) for e in range(xc.CROSS_E)]
    print("cross min_gap %.3g" % min(r["stats"]["min_gap"] for r in runs), [r["total_steps"] for r in runs], [r["stats"]["changed"] for r in runs])
    for e, (r, (name, (eps, h))) in enumerate(zip(runs, pairs)):
        assert r["stats"]["min_gap"] >= hc.MIN_GAP, (e, pairs[e], r["stats"])
        assert eps == 0 or r["stats"]["changed"] >= 5, (e, r["stats"])
        assert r["episodes"] > h
    assert xc.cross_chain(2, "thr0", (0.3, 4))["stats"]["min_gap"] < hc.MIN_GAP


def test_the_demo_case_at_the_demos_ids():
    """frirl_demo numbers its agents from 0 unless --id-base says otherwise.  At ids 0 .. 8 seed 1265 does NOT keep the margin (min gap
    1.9e-7 at agent 1, 3.9e-7 at agent 2: below MIN_GAP), so tests/test_hip_explore_rows.py runs the demo with --id-base 77, the
    admitted case above; this test keeps the reason on record."""
    gaps = [xc.agent_run("mountaincar", e, id_base=0)["stats"]["min_gap"] for e in range(9)]
    print("ids 0..8 min gaps", ["%.3g" % g for g in gaps])
    assert min(gaps) < hc.MIN_GAP <= min(xc.agent_run("mountaincar", e)["stats"]["min_gap"] for e in range(9))


@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_point_cases_stay_under_the_near_tie_cap(nant, A):
    """A dry run of the mirrors of the caller-stepped case (the reference alone, 16 agents, 5 episodes, epsilon 0.4 over horizon
    e mod 4): picks at which the two best conclusions lie within 1e-12 relative are at most a tenth of the picks, the cap on picks
    that may follow the device; episodes cross every horizon, and every agent explored.
    Measured near-ties / picks: 2 x 32 18 / 706, 4 x 5 25 / 2919, 8 x 3 19 / 3174 (at most 2.5 %).  The 2 x 32 shape runs on
    explore_rows_cases.point_description: under point_desc's action universe only 21 of the 32 actions have a point of their own,
    two actions on one point conclude the same bit for bit, and 190 of 692 picks had such a pair on top (27 %, and 15.8 % at best
    over 360 choices of stream and start-state seeds) -- a degenerate description, not a property of the picks."""
    from tests.test_hip_explore_rows import point_mirrors
    env, starts, mirrors = point_mirrors(nant, A)
    assert len(set(xc.point_description(nant, A)["action_ve"].tolist())) == A, "every action a point of its own in the action universe"
    for ep in range(1, xc.POINT_EPISODES + 1):
        for m in mirrors:
            if not m.converged:
                m.explore_episode(env, None, ep)
    near, picks = sum(m.near for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, "near", near, "picks", picks, "explored", [m.explored for m in mirrors])
    assert near * 10 <= picks, (near, picks)
    assert all(m.explored > 0 for m in mirrors)
