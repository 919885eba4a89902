"""The exploring cases of tests/test_hip_explore.py, computed by the oracle alone (no GPU): the GPU tests compare the kernels with
these, and tests/test_explore_ref.py checks on the CPU that the cases are worth comparing with (enough exploring picks that change
the action, no near-tie at a greedy pick, enough parked rows).

Learning: the three demos with the portable trig, E environments from the demo's start state with global ids BASE .. BASE + E - 1,
so the trajectories differ through their streams only.  Roll-outs: Q rows on the oracle's converged rule base, ids BASE .. BASE + Q - 1.
"""
import ctypes as C
import functools

import numpy as np

from oracle import binding as ob

DEMOS = ["mountaincar", "cartpole", "acrobot"]
BASE, EPSILON = 77, 0.3
# Seed 1234 everywhere except mountaincar: there the oracle alone, on the learning case, has a greedy pick whose two best conclusions
# are 1.6e-16 apart (equal in real arithmetic) in environment 0 -- as have 1238, 1241, 1243, 1244 and 1245; 1235 is the next without.
SEEDS = {"mountaincar": 1235, "cartpole": 1234, "acrobot": 1234}
E, MAXR, EPISODES, MAX_STEPS = 8, 512, 3, 120
Q = 64
ROLLOUT_MAX_STEPS = 200          # roll-outs on the trained base: long enough that rows outlive ROLLOUT_CAP
ROLLOUT_CAP = 32                 # steps before the staged roll-out parks a row ("rollout_cap")
MASKS = [0, 1, 0xffff, 0xa5a5a5a5]      # try-remove masks, row q carries MASKS[q % 4]

TRACE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


def exploring_oracle(env, e, max_steps=MAX_STEPS):
    fr = ob.Frirl(env, trig_mode=1, maxR=MAXR)
    fr.set_max_steps(max_steps)
    fr.set_exploration(EPSILON, 0, SEEDS[env], BASE + e)
    return fr


def snapshot(fr):
    f = fr.five
    R = f.R
    return dict(steps=fr.ep_steps, reward=fr.ep_reward, R=R, rant=np.array(f.rant[:R]), rconc=np.array(f.rconc[:R]), veval=np.array(f.veval[:, :R]),
                uidx=np.array(f.uidx[:, :R]), fus=int(fr.fus), states=fr.last_states)


@functools.lru_cache(maxsize=None)
def learning_case(env):
    """EPISODES exploring episodes of E environments.  Returns (episodes, stats): episodes[ep][e] = dict(first = value of the first
    action, trace = [(action value taken, state after it, quantised state + next action, rule count before the update)], end =
    snapshot after the episode); stats[e] = the oracle's exploration counters."""
    frs = [exploring_oracle(env, e) for e in range(E)]
    episodes = []
    for ep in range(EPISODES):
        row = []
        for fr in frs:
            ns, nant, f = fr.nstates, fr.nant, fr.five
            trace = []

            def cb(frp, step, action, cur_states, cur_q, ud):
                trace.append((action, np.array([cur_states[i] for i in range(ns)]), np.array([cur_q[i] for i in range(nant)]), f.R))
            cbo = TRACE_FN(cb)
            ob.lib().orc_frirl_set_trace(fr.h, cbo)
            fr.episode()
            ob.lib().orc_frirl_set_trace(fr.h, None)
            row.append(dict(first=trace[0][0], trace=trace, end=snapshot(fr)))
        episodes.append(row)
    return episodes, [fr.explore_stats for fr in frs]


@functools.lru_cache(maxsize=None)
def construct_case(env):
    """The same environments through the oracle's construct loop (orc_sequential_run) with max_episodes = EPISODES + 1, i.e. at most
    EPISODES episodes.  Returns per environment dict(converged, episodes, total_steps, end = snapshot, stats)."""
    out = []
    for e in range(E):
        fr = exploring_oracle(env, e)
        ok = fr.run(max_episodes=EPISODES + 1)
        out.append(dict(converged=ok, episodes=fr.rng_episode, total_steps=fr.total_steps, end=snapshot(fr), stats=fr.explore_stats))
    return out


def trained(env):
    fr = ob.Frirl(env, trig_mode=1)
    assert fr.run() == 1
    return fr


def rollout_starts(fr, n, seed=5):
    """Start states around the demo's own (as tests/test_hip_shared.py: start_states); row 0 is the demo's."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, fr.nstates))
    for k in range(fr.nstates):
        d = fr.dim(k)
        vals = d["values"]
        s[:, k] = np.clip(d["values_def"] + rng.uniform(-0.15, 0.15, n) * (vals[-1] - vals[0]), vals[0], vals[-1])
        s[0, k] = d["values_def"]
    return s


def mask_candidates(fr):
    """Slots 0..15: the rules of largest |Q|, 16..31: of smallest (as tests/test_hip_shared.py)."""
    R = fr.five.R
    order = np.argsort(np.abs(fr.five.rconc[:R]), kind="stable")
    return [int(r) for r in order[-16:][::-1]] + [int(r) for r in order[:16]]


@functools.lru_cache(maxsize=None)
def rollout_case(env, masked):
    """Q exploring roll-outs (episode key 0) of ROLLOUT_MAX_STEPS steps at most on the converged rule base; with `masked`, row q runs
    on the base without the candidate rules of MASKS[q % 4].  Returns dict(starts, steps, reward, success, final, stats[q])."""
    base = trained(env)
    cand = mask_candidates(base)
    s = rollout_starts(base, Q)
    frs = {}
    for m in (MASKS if masked else [0]):
        fr = trained(env)
        for r in sorted([cand[sl] for sl in range(32) if (m >> sl) & 1], reverse=True):
            fr.five.remove_rule(r)
        fr.set_max_steps(ROLLOUT_MAX_STEPS)
        frs[m] = fr
    steps, reward, success, final, stats = np.zeros(Q, np.int32), np.zeros(Q), np.zeros(Q, np.int32), np.zeros((Q, base.nstates)), []
    for q in range(Q):
        fr = frs[MASKS[q % 4] if masked else 0]
        before = fr.explore_stats
        fr.set_start_state(s[q])
        fr.set_exploration(EPSILON, 0, SEEDS[env], BASE + q)
        fr.episode_eval()
        steps[q], reward[q], success[q], final[q] = fr.ep_steps, fr.ep_reward, fr.success, fr.last_states
        after = fr.explore_stats
        stats.append(dict({k: after[k] - before[k] for k in ("picks", "explored", "changed", "clamped")}, min_gap=after["min_gap"]))
    return dict(starts=s, steps=steps, reward=reward, success=success, final=final, stats=stats, cand=cand, R=base.five.R)
