"""Cases of the per-agent exploration rows (frirl_hip_explore_rows): agent e of a batch explores at its own epsilon, annealed
linearly to zero over its own horizon.  No GPU needed; tests/test_explore_rows_ref.py asserts on the oracle alone that the cases are
worth running, tests/test_hip_explore_rows.py runs them on the device.

The reference of agent e is the oracle's own construct loop, one episode per call: Frirl.set_exploration(rate of episode k, 0, seed,
id, episode=k - 1) followed by Frirl.run(max_episodes=2) runs exactly episode k with the loop's convergence bookkeeping, the previous
episode's steps, reward and consequents staying in the oracle object between calls.
"""
import functools
import struct

import numpy as np

from oracle import binding as ob
from tests import hparams_cases as hc

ID_BASE = 77            # global id of agent e: ID_BASE + e (frirl_hip_agent.env_id_base)
MAXR = 512
HORIZON_MAX = 2 ** 30

# demo -> (agents, (epsilon, horizon) sets, seed, max_episodes); agent e explores under set e mod nsets
CASES = {
    "mountaincar": (9, [(0.0, 0), (0.1, 2), (0.3, 4)], 1265, 40),
    "acrobot": (12, [(0.0, 0), (0.1, 2), (0.3, 4), (0.3, 0)], 1234, 10),
    "cartpole": (12, [(0.0, 0), (0.1, 2), (0.3, 4), (0.3, 0)], 1234, 8),
}
DEMOS = list(CASES)
# what the oracle gave when the cases were chosen; tests/test_explore_rows_ref.py re-asserts it
MEASURED = {
    "mountaincar": dict(converged=[1, 0, 1, 1, 1, 0, 1, 1, 1], episodes=[29, 39, 35, 29, 24, 39, 29, 24, 35], total_steps=149172),
    "acrobot": dict(converged=[0] * 12, episodes=[9] * 12, total_steps=19007),
    "cartpole": dict(converged=[0] * 12, episodes=[7] * 12, total_steps=4897),
}


def epsilon_at(eps, horizon, episode):
    """The contract's rate (include/frirl_hip.h) in Python's correctly rounded float64: one division, then one multiplication."""
    if horizon == 0:
        return eps
    if episode > horizon:
        return 0.0
    return eps * (float(horizon - (episode - 1)) / float(horizon))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def agent_sets(env):
    E, sets, _, _ = CASES[env]
    return [sets[e % len(sets)] for e in range(E)]


def chain(env, gid, seed, max_episodes, rate, hparams=None, maxR=MAXR):
    """The oracle's construct loop of one agent, an episode per call, exploring at rate(k) in episode k = 1 .. max_episodes - 1:
    dict(fr, converged, episodes, total_steps, stats).  hparams: a set name of hparams_cases.SETS."""
    fr = hc.demo_frirl(env, hparams or "default", trig_mode=1, maxR=maxR)
    converged, episodes = 0, 0
    for k in range(1, max_episodes):
        fr.set_exploration(rate(k), 0, seed, gid, episode=k - 1)
        converged = int(fr.run(max_episodes=2))
        episodes = k
        if converged:
            break
    return dict(fr=fr, converged=converged, episodes=episodes, total_steps=fr.total_steps, stats=fr.explore_stats)


@functools.lru_cache(maxsize=None)
def agent_run(env, e, under=None, id_base=ID_BASE, hparams=None):
    """Agent e of the demo's case under its own set (or under set index `under`).  Cached: the Frirl object is shared, read it only."""
    E, sets, seed, max_episodes = CASES[env]
    eps, h = sets[(e if under is None else under) % len(sets)]
    return chain(env, id_base + e, seed, max_episodes, lambda k: epsilon_at(eps, h, k), hparams=hparams)


def columns(pairs):
    """Host columns for one (epsilon, horizon) pair per agent."""
    return dict(epsilon=np.array([p[0] for p in pairs], dtype=np.float64), horizon=np.array([p[1] for p in pairs], dtype=np.int32))


# ---- the rows crossed with hyper-parameter rows (acrobot): agent e under hyper-parameter set e mod 6 of the rows test's demo sets and
# exploration set e mod 4, over the eight episodes those sets are admitted for (hparams_cases.TRAJ_EPISODES).  One pairing is left to
# the greedy set: with weight_significant = 0 ("thr0") every update spreads to every rule, and once an exploratory pick has been
# learned the two best conclusions tie to 1e-16 relative (tests/test_explore_rows_ref.py asserts it), so thr0 explores under set 0.
CROSS_ENV, CROSS_E = "acrobot", 12
CROSS_EPISODES = hc.TRAJ_EPISODES[CROSS_ENV]


def cross_sets():
    from tests import hparam_rows_cases as rc
    hsets = rc.demo_sets(CROSS_ENV)
    xsets = CASES[CROSS_ENV][1]
    return [(hsets[e % len(hsets)], xsets[0 if hsets[e % len(hsets)] == "thr0" else e % len(xsets)]) for e in range(CROSS_E)]


def cross_chain(e, name, pair):
    eps, h = pair
    return chain(CROSS_ENV, ID_BASE + e, CASES[CROSS_ENV][2], CROSS_EPISODES, lambda k: epsilon_at(eps, h, k), hparams=name)


@functools.lru_cache(maxsize=None)
def cross_run(e):
    return cross_chain(e, *cross_sets()[e])


# ---- caller-stepped agents on the point environment: agent e with epsilon 0.4 and horizon e mod 4 -----------------------------------------
POINT_SHAPES = [(2, 32), (4, 5), (8, 3)]
POINT_E, POINT_EPISODES, POINT_MAXR, POINT_EPS, POINT_SEED = 16, 5, 1024, 0.4, 4321


def point_pairs():
    return [(POINT_EPS, e % 4) for e in range(POINT_E)]


def point_description(nant, A):
    """tests/test_hip_external.py::point_desc wherever its action universe (step 0.1, 41 points) tells the actions apart.  With 32
    actions it does not: they lie 0.0645 apart, only 21 of the 32 get a universe point of their own, and two actions on one point
    are one antecedent to the rule base, so their conclusions are equal bit for bit at every pick (190 of 692 picks of the case had
    such a pair on top).  For that shape the same grids, hyper-parameters and environment with an action universe of step 0.03 and
    81 points per universe (the state universes then reach +-2.4 instead of +-1.2, their step unchanged): 32 distinct points."""
    import frirl_amd
    from tests.test_hip_external import point_desc
    if 2.0 / (A - 1) >= 0.2:
        return point_desc(nant, A)
    base = point_desc(nant, A)
    ns = nant - 1
    states = [dict(values=base["grids"][k], div=base["grid_div"][k], steep=1.0 + 0.5 * (k % 2), default=0.0, universe_div=0.06) for k in range(ns)]
    actions = dict(values=base["grids"][ns], div=base["grid_div"][ns], universe_div=0.03)
    return frirl_amd.describe(states, actions, 81, base["alpha"], base["gamma"], base["qdiff_pos"], base["qdiff_neg"], weight_thr=base["weight_thr"],
                              skip_rules=base["skip_rules"], reward_good_above=base["reward_good_above"], qdiff_final_tolerance=base["qdiff_final_tolerance"],
                              max_steps=base["max_steps"], name=f"point{nant}x{A}")
