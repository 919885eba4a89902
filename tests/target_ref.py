"""Reference of the per-agent TD target (frirl_hip_target_rows): SARSA learns towards Q(s', a') of the action taken, Q-learning towards
Q(s', g) of the greedy action the pick started from.  No GPU needed; tests/test_target_ref.py asserts on the oracle alone that the cases
are worth running, tests/test_hip_target.py runs them on the device.

The oracle is not changed.  Its own loop cannot give the update another point than the one the episode goes on from, so one agent's
construct loop is restated here step by step from the oracle's exported pieces: Frirl.get_best_action, oracle.binding.e_greedy_pick at
the rate explore_rows_cases.epsilon_at, Frirl.env_step, Frirl.update_sarsa(q_ant, reward, (q(s'), value of g or of a')) and the loop's
convergence bookkeeping as tests/test_hip_external.py::Mirror.episode keeps it.  With target SARSA the restated loop is the oracle's
(tests/test_target_ref.py compares it with explore_rows_cases.chain bit for bit).
"""
import functools

import numpy as np

from oracle import binding as ob
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests.teach_ref import TaughtMirror

SARSA, Q = 0, 1                 # FRIRL_HIP_TARGET_SARSA / _Q
MAX_STEPS = 1000                # of every demo (oracle/frirl_oracle.c: orc_frirl_config)
# episodes per demo: max_episodes of the construct loop is one more
EPISODES = {"mountaincar": 8, "acrobot": 9, "cartpole": 7}
DEMOS = list(EPISODES)


def relative_gap(oc, greedy):
    """The oracle's statistic (orc_e_greedy): relative gap between the conclusion of the greedy action and the best of the others, or
    None for a pair with equal bits (both sides take the first maximum there)."""
    others = [oc[a] for a in range(len(oc)) if a != greedy]
    if not others:
        return None
    best, second = float(oc[greedy]), float(max(others))
    if xc.bits(best) == xc.bits(second):
        return None
    return (best - second) / max(abs(best), abs(second))


def chain(env, gid, seed, max_episodes, rate, target, hparams=None, maxR=xc.MAXR):
    """One agent's construct loop, episodes 1 .. max_episodes - 1, exploring at rate(k) in episode k and learning towards `target`.
    dict(fr, converged, episodes, total_steps, ep_steps, ep_reward, stats); stats: picks, explored (random branch), changed (g != a'),
    min_gap over the picks that stayed greedy (NaN: none)."""
    fr = hc.demo_frirl(env, hparams or "default", trig_mode=1, maxR=maxR)
    hp, f = fr.hparams, fr.five
    ns, A = fr.nstates, fr.nactions
    av = fr.dim(ns)["values"]
    start = np.array([fr.dim(k)["values_def"] for k in range(ns)])
    stats = dict(picks=0, explored=0, changed=0, min_gap=float("nan"))

    def pick(states, episode, step):
        """(g, a'): frirl_get_best_action, then frirl_e_greedy_selection on the stream of (seed, gid, episode, step)."""
        g = fr.get_best_action(states)
        a = ob.e_greedy_pick(g, A, rate(episode), 0, seed, gid, episode, step)
        stats["picks"] += 1
        # the random branch is taken exactly when the first draw does not exceed a non-zero rate (orc_e_greedy_pick)
        eps = rate(episode)
        if eps != 0.0 and not ob.rng_unit(seed, gid, episode, step, 0) > eps:
            stats["explored"] += 1
            stats["changed"] += int(a != g)
        else:
            gap = relative_gap(fr.actconc, g)
            if gap is not None and not stats["min_gap"] <= gap:
                stats["min_gap"] = gap
        return g, a

    converged, episodes, total_steps = 0, 0, 0
    ep_steps, ep_reward = 0, 0.0                                     # frirl_sequential_run.c: the previous episode's, 0 before the first
    for k in range(1, max_episodes):
        prev_R, prev_steps, prev_reward = f.R, ep_steps, ep_reward    # :68-72
        prev_q = np.array(f.rconc[: f.maxR]).copy()
        states = start.copy()                                        # frirl_episode.c:46-48: the un-quantised default state
        _, a0 = pick(states, k, 0)                                   # :78 -- no update at the first action
        q_ant = np.concatenate([states, [av[a0]]])
        ep_steps, ep_reward = 0, 0.0
        for step in range(1, MAX_STEPS + 1):
            cur, reward, success, q = fr.env_step(q_ant[ns], states)
            ep_reward += reward
            g, a = pick(q, k, step)
            cur_q_ant = np.concatenate([q, [av[a]]])                 # the episode goes on from (s', a')
            towards = np.concatenate([q, [av[g if target == Q else a]]])
            fr.update_sarsa(q_ant, reward, towards)
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


def rule_base(fr):
    """(R, antecedent bytes, consequent bytes) of an oracle agent."""
    R = fr.five.R
    return R, np.array(fr.five.rant[:R]).tobytes(), np.array(fr.five.rconc[:R]).tobytes()


@functools.lru_cache(maxsize=None)
def agent_run(env, e, target):
    """Agent e of explore_rows_cases.CASES[env] (its set, seed and id) over EPISODES[env] episodes under `target`.  Cached: read only."""
    E, sets, seed, _ = xc.CASES[env]
    eps, h = sets[e % len(sets)]
    return chain(env, xc.ID_BASE + e, seed, EPISODES[env] + 1, lambda k: xc.epsilon_at(eps, h, k), target)


def mixed_column(env):
    """A target per agent such that every (epsilon, horizon) set of the case occurs under both targets: the sets repeat with period
    nsets, the targets with period 2 * nsets."""
    E, sets, _, _ = xc.CASES[env]
    col = np.array([(e // len(sets)) % 2 for e in range(E)], dtype=np.uint8)
    assert {(e % len(sets), int(col[e])) for e in range(E)} == {(s, t) for s in range(len(sets)) for t in (SARSA, Q)}
    return col


# ---- the rows crossed with hyper-parameter rows: explore_rows_cases' acrobot cross case, target e mod 2 ---------------------------------
def cross_column():
    return np.array([e % 2 for e in range(xc.CROSS_E)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cross_run(e):
    name, (eps, h) = xc.cross_sets()[e]
    return chain(xc.CROSS_ENV, xc.ID_BASE + e, xc.CASES[xc.CROSS_ENV][2], xc.CROSS_EPISODES, lambda k: xc.epsilon_at(eps, h, k), int(cross_column()[e]), hparams=name)


# ---- caller-stepped agents --------------------------------------------------------------------------------------------------------------
class TargetMirror(TaughtMirror):
    """tests/teach_ref.py::TaughtMirror that explores at the rate of the episode (as tests/test_hip_explore_rows.py::ExploreMirror does)
    and, under target Q, hands the update (q(s'), value of g) instead of (q(s'), value of a').  Mirror.episode calls the oracle's update
    directly, so the episode is restated here with that one vector changed.  g is the oracle's greedy action; where the pick itself
    stayed greedy it is the pick (which may follow the device inside Mirror.pick's 1e-12 tie)."""

    def __init__(self, d, start, maxR, eps, horizon, seed, gid, target, teacher=None):
        super().__init__(d, start, maxR, explore=dict(epsilon=eps, seed=seed), gid=gid, teacher=teacher)
        self.eps, self.horizon, self.target = eps, horizon, target
        self.off_policy = 0            # learning steps with g != a'
        self.step_no = 0

    def pick(self, states, device_pick, step=0):
        g, _ = self.five.best_action(states, self.d["action_ve"])
        before = (self.taught, self.explored)
        a = super().pick(states, device_pick, step)
        self.g = a if (self.taught, self.explored) == before else g
        return a

    def target_episode(self, env, picks, key):
        """The episode whose stream key is `key`: Mirror.episode with the update towards (q(s'), value of g) under target Q."""
        from tests.test_hip_external import generic_quantize
        assert key == self.episode_no + 1
        self.explore["epsilon"] = xc.epsilon_at(self.eps, self.horizon, key)
        d, f = self.d, self.five
        NS = d["nant"] - 1
        av = d["grids"][NS]
        self.prev["R"], self.prev["q"] = f.R, np.array(f.rconc[: f.maxR]).copy()
        self.episode_no += 1
        states = self.start.copy()
        picks = picks if picks is not None else [None] * (d["max_steps"] + 1)
        a0 = self.pick(states, picks[0], 0)
        q_ant = np.concatenate([states, [av[a0]]])
        actions, steps, total = [a0], 0, 0.0
        while True:
            x, r, ok = env.step(np, states[None], np.array([q_ant[NS]]))
            cur, r, success = x[0], float(r[0]), int(ok[0])
            q = generic_quantize(d, cur)
            a = self.pick(q, picks[steps + 1], steps + 1)
            self.off_policy += int(a != self.g)
            cur_q_ant = np.concatenate([q, [av[a]]])
            towards = np.concatenate([q, [av[self.g if self.target == Q else a]]])
            self.learn(q_ant, r, towards)
            states, q_ant = cur, cur_q_ant
            steps += 1
            total += r
            actions.append(a)
            if success == 1 or steps >= d["max_steps"]:
                break
        same = self.prev["R"] == f.R and self.prev["steps"] == steps and total > d["reward_good_above"] and self.prev["reward"] == total
        if same and not (np.abs(np.array(f.rconc[: f.R]) - self.prev["q"][: f.R]) >= d["qdiff_final_tolerance"]).any():
            self.converged = True
        self.prev["steps"], self.prev["reward"] = steps, total
        return actions, steps, total


def scripted_teacher(e, A):
    """Agent e's teacher of the taught point case: an action at two steps in three, `choose yourself` (-1) otherwise."""
    return lambda step: -1 if (step + e) % 3 == 0 else (step * 5 + e * 3) % A


def point_targets():
    """Target of agent e of the point case: the (epsilon, horizon) pairs repeat with period 4 (explore_rows_cases.point_pairs), the
    targets with period 8, so that every horizon occurs under both."""
    return np.array([(e // 4) % 2 for e in range(xc.POINT_E)], dtype=np.uint8)


def point_mirrors(nant, A, taught):
    """Environment, start states and one TargetMirror per agent of the caller-stepped case (no GPU needed)."""
    from tests.test_hip_external import PointEnv
    d = xc.point_description(nant, A)
    starts = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, (xc.POINT_E, nant - 1)))
    tq = point_targets()
    mirrors = [TargetMirror(d, starts[e], xc.POINT_MAXR, eps, h, xc.POINT_SEED, xc.ID_BASE + e, int(tq[e]), teacher=scripted_teacher(e, A) if taught else None)
               for e, (eps, h) in enumerate(xc.point_pairs())]
    return PointEnv(nant - 1), starts, mirrors
