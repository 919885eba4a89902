"""Reference of per-agent expected SARSA (frirl_hip_expect_rows): a flagged agent learns towards the expectation v of the A conclusions
at s' under what its epsilon-greedy pick really does.  No GPU needed; tests/test_expect_ref.py asserts on the oracle alone that the cases
are worth running, tests/test_hip_expect.py runs them on the device.

The oracle is not changed.  Its update forms  alpha * (reward + gamma * Q(cur_q_ant) - Q(q_ant));  called with gamma 0 and the reward
reward + gamma * v  it is the update towards an arbitrary value v, everything else -- insertion test, snap, append, spread, sticky flag --
being its own code.  One agent's construct loop is tests/target_ref.py::chain with the update replaced by that restatement: with
v = Q(s', a') it ends on chain(target=SARSA) bit for bit, with v = Q(s', g) on chain(target=Q) (tests/test_expect_ref.py).
"""
import functools

import numpy as np

from oracle import binding as ob
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests import target_ref as tr

SARSA, Q, EXPECTED = 0, 1, 2        # the value the restated update learns towards
# mountaincar under its own seed 1265 does not keep hparams_cases.MIN_GAP under the mixed column (expected agent 2: 8.9e-7)
SEEDS = {"mountaincar": 1266, "acrobot": 1234, "cartpole": 1234}
DEMOS = tr.DEMOS


def expected_value(c, g, eps):
    """The contract's value (include/frirl_hip.h) in Python's float64, every operation rounded on its own, in the contract's order."""
    A = len(c)
    if eps == 0.0:
        return float(c[g])
    S = float(c[0])
    for a in range(1, A):
        S = S + float(c[a])
    M = (S - 0.5 * float(c[0])) + 0.5 * float(c[A - 1])
    return (1.0 - eps) * float(c[g]) + (eps / A) * M


def chain(env, gid, seed, max_episodes, rate, mode, hparams=None, maxR=xc.MAXR):
    """tests/target_ref.py::chain with the gamma-0 restatement of the update: one agent's construct loop, episodes 1 .. max_episodes - 1,
    exploring at rate(k) in episode k and learning towards Q(s', a') (SARSA), Q(s', g) (Q) or the expectation (EXPECTED).
    dict(fr, converged, episodes, total_steps, ep_steps, ep_reward, stats); stats as target_ref.chain's, and value_differs: learning
    steps at which the value differs from Q(s', a') in bits."""
    fr = hc.demo_frirl(env, hparams or "default", trig_mode=1, maxR=maxR)
    hp, f = dict(fr.hparams), fr.five
    gamma = float(hp["gamma"])
    fr.set_hparams(gamma=0.0)
    ns, A = fr.nstates, fr.nactions
    av = fr.dim(ns)["values"]
    start = np.array([fr.dim(k)["values_def"] for k in range(ns)])
    stats = dict(picks=0, explored=0, changed=0, min_gap=float("nan"), value_differs=0)

    def pick(states, episode, step):
        g = fr.get_best_action(states)
        eps = rate(episode)
        a = ob.e_greedy_pick(g, A, eps, 0, seed, gid, episode, step)
        stats["picks"] += 1
        if eps != 0.0 and not ob.rng_unit(seed, gid, episode, step, 0) > eps:
            stats["explored"] += 1
            stats["changed"] += int(a != g)
        else:
            gap = tr.relative_gap(fr.actconc, g)
            if gap is not None and not stats["min_gap"] <= gap:
                stats["min_gap"] = gap
        return g, a, np.array(fr.actconc).copy()

    converged, episodes, total_steps = 0, 0, 0
    ep_steps, ep_reward = 0, 0.0
    for k in range(1, max_episodes):
        prev_R, prev_steps, prev_reward = f.R, ep_steps, ep_reward
        prev_q = np.array(f.rconc[: f.maxR]).copy()
        states = start.copy()
        _, a0, _ = pick(states, k, 0)
        q_ant = np.concatenate([states, [av[a0]]])
        ep_steps, ep_reward = 0, 0.0
        for step in range(1, tr.MAX_STEPS + 1):
            cur, reward, success, q = fr.env_step(q_ant[ns], states)
            ep_reward += reward
            g, a, c = pick(q, k, step)
            cur_q_ant = np.concatenate([q, [av[a]]])
            v = float(c[a]) if mode == SARSA else float(c[g]) if mode == Q else expected_value(c, g, rate(k))
            stats["value_differs"] += int(xc.bits(v) != xc.bits(c[a]))
            fr.update_sarsa(q_ant, reward + gamma * v, cur_q_ant)          # gamma is 0: the update towards v
            states, q_ant = cur, cur_q_ant
            ep_steps += 1
            total_steps += 1
            if success == 1:
                break
        episodes = k
        if prev_R == f.R and prev_steps == ep_steps and ep_reward > hp["reward_good_above"] and prev_reward == ep_reward and \
                not (np.abs(np.array(f.rconc[: f.R]) - prev_q[: f.R]) >= hp["qdiff_final_tolerance"]).any():
            converged = 1
            break
    return dict(fr=fr, converged=converged, episodes=episodes, total_steps=total_steps, ep_steps=ep_steps, ep_reward=ep_reward, stats=stats)


def agent_set(env, e):
    sets = xc.CASES[env][1]
    return sets[e % len(sets)]


@functools.lru_cache(maxsize=None)
def agent_run(env, e, mode, seed=None):
    """Agent e of explore_rows_cases.CASES[env] (its set and id) under SEEDS[env] over target_ref.EPISODES[env] episodes.  Cached: read only."""
    eps, h = agent_set(env, e)
    return chain(env, xc.ID_BASE + e, SEEDS[env] if seed is None else seed, tr.EPISODES[env] + 1, lambda k: xc.epsilon_at(eps, h, k), mode)


def mixed_column(env):
    """expected[e] = (e // nsets) % 2: every agent is SARSA or expected, and every (epsilon, horizon) set occurs under both."""
    E, sets, _, _ = xc.CASES[env]
    col = np.array([(e // len(sets)) % 2 for e in range(E)], dtype=np.uint8)
    assert {(e % len(sets), int(col[e])) for e in range(E)} == {(s, t) for s in range(len(sets)) for t in (0, 1)}
    return col


def mode_of(flag):
    return EXPECTED if flag else SARSA


# ---- crossed with hyper-parameter rows: explore_rows_cases' acrobot cross case, flag e mod 2 where the agent is admitted ------------------
# the agents of the cross case whose expected chain falls below hparams_cases.MIN_GAP and therefore stay on SARSA: none (the smallest gap of
# the column e mod 2 is 1.06e-6).  tests/test_expect_ref.py asserts that the admission still gives exactly this list.
CROSS_LEFT_ON_SARSA = ()


def cross_wanted():
    return np.array([e % 2 for e in range(xc.CROSS_E)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cross_run(e, mode):
    name, (eps, h) = xc.cross_sets()[e]
    return chain(xc.CROSS_ENV, xc.ID_BASE + e, xc.CASES[xc.CROSS_ENV][2], xc.CROSS_EPISODES, lambda k: xc.epsilon_at(eps, h, k), mode, hparams=name)


@functools.lru_cache(maxsize=None)
def cross_column():
    """Flag e mod 2, except that an agent whose expected chain falls below hparams_cases.MIN_GAP stays on SARSA (MIN_GAP is not loosened)."""
    col = cross_wanted().copy()
    for e in range(xc.CROSS_E):
        if col[e] and not cross_run(e, EXPECTED)["stats"]["min_gap"] >= hc.MIN_GAP:
            col[e] = 0
    return col


# ---- caller-stepped agents ------------------------------------------------------------------------------------------------------------------
class ExpectMirror(tr.TargetMirror):
    """tests/target_ref.py::TargetMirror whose flagged agent learns towards the expectation: the update goes through an ob.Agent whose gamma
    is 0, with the reward  reward + gamma * v.  An unflagged agent is the TargetMirror under SARSA.  The conclusions are the oracle's at
    the pick; g is TargetMirror's (the pick itself where it stayed greedy, which may follow the device inside Mirror.pick's 1e-12 tie)."""

    def __init__(self, d, start, maxR, eps, horizon, seed, gid, expected, teacher=None):
        super().__init__(d, start, maxR, eps, horizon, seed, gid, tr.SARSA, teacher=teacher)
        self.expected = int(expected)
        self.gamma = float(d["gamma"])
        self.oa0 = ob.Agent(d["alpha"], 0.0, d["qdiff_pos"], d["qdiff_neg"], d["weight_thr"], d["skip_rules"], d["grids"])
        self.value_differs = 0

    def pick(self, states, device_pick, step=0):
        _, self.c = self.five.best_action(states, self.d["action_ve"])
        self.c = np.array(self.c).copy()
        return super().pick(states, device_pick, step)

    def learn(self, q_ant, reward, cur_q_ant):
        if not self.expected:
            return super().learn(q_ant, reward, cur_q_ant)
        a = int(np.argmin(np.abs(self.d["grids"][self.d["nant"] - 1] - cur_q_ant[-1])))
        v = expected_value(self.c, self.g, self.explore["epsilon"])
        self.value_differs += int(xc.bits(v) != xc.bits(self.c[a]))
        oa, self.oa = self.oa, self.oa0
        try:
            return super().learn(q_ant, reward + self.gamma * v, cur_q_ant)
        finally:
            self.oa = oa


def point_flags():
    """Flag of agent e of the point case: the (epsilon, horizon) pairs repeat with period 4, the flags with period 8."""
    return np.array([(e // 4) % 2 for e in range(xc.POINT_E)], dtype=np.uint8)


def point_mirrors(nant, A, taught):
    """Environment, start states and one ExpectMirror per agent of the caller-stepped case (no GPU needed)."""
    from tests.test_hip_external import PointEnv
    d = xc.point_description(nant, A)
    starts = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, (xc.POINT_E, nant - 1)))
    xf = point_flags()
    mirrors = [ExpectMirror(d, starts[e], xc.POINT_MAXR, eps, h, xc.POINT_SEED, xc.ID_BASE + e, int(xf[e]), teacher=tr.scripted_teacher(e, A) if taught else None)
               for e, (eps, h) in enumerate(xc.point_pairs())]
    return PointEnv(nant - 1), starts, mirrors
