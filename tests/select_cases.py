"""CPU side of the selection tests on the batch object: the oracle's reference of a clone that keeps its own hyper-parameter row.

Such a clone is ONE oracle agent whose hyper-parameters change between episodes: hc.demo_frirl(env, a) runs k single episodes
(Frirl.run(max_episodes=2): one episode of the construct loop, the bookkeeping staying in the object between calls), set_hparams
switches it to set b (the description's own values, then hc.overrides(b, ...)), and m more single episodes follow.  The source of
the clone is the chain a -> a.  No GPU needed; tests/test_select_ref.py asserts on the oracle alone that the cases are worth running,
tests/test_hip_select.py runs them on the device.
"""
import functools

import numpy as np

from oracle import binding as ob
from tests import hparams_cases as hc

MAXR = 512
# (env, a, b, k, m): agents under a and b learn k episodes, the one under b is replaced by a copy of the one under a, m more episodes
CASES = [
    ("mountaincar", "thr_small", "noskip_thr_small_tight", 5, 5),
    ("mountaincar", "noskip_thr_small_tight", "thr_small", 5, 5),
    ("mountaincar", "default", "thr_small", 5, 5),
    ("mountaincar", "thr_small", "default", 5, 5),
    ("acrobot", "noskip", "thr_big", 4, 3),
    ("acrobot", "alpha_gamma", "thr0", 4, 3),
    ("acrobot", "thr_big", "noskip", 4, 3),
    ("acrobot", "default", "alpha_gamma", 4, 3),
    ("cartpole", "noskip", "thr_small", 3, 2),
]
ENVS = ["mountaincar", "acrobot", "cartpole"]
EPISODES = {"mountaincar": (5, 5), "acrobot": (4, 3), "cartpole": (3, 2)}          # (k, m) of every case of the demo
UNTOUCHED = {"mountaincar": "noskip_thr_small_tight", "acrobot": "thr0", "cartpole": "thr_big"}      # an agent nobody clones, under one of hc.TRAJ_CASES


def env_cases(env):
    return [c for c in CASES if c[0] == env]


@functools.lru_cache(maxsize=None)
def chain(env, a, b, k, m):
    """The oracle's k episodes under set a, then m under set b: dict(fr, converged (any call said so), records = per episode
    (rules, steps, reward), stats = explore_stats).  Cached: the Frirl object is shared, read it only."""
    fr = hc.demo_frirl(env, a, trig_mode=1, maxR=MAXR)
    own = {key: ob.Frirl(env, trig_mode=1, maxR=MAXR).hparams[key] for key in hc.HP_KEYS}
    converged, records = 0, []
    for i in range(k + m):
        if i == k and b != a:
            fr.set_hparams(**dict(own, **hc.overrides(b, own)))
        converged |= int(fr.run(max_episodes=2))
        records.append((fr.five.R, fr.ep_steps, fr.ep_reward))
    return dict(fr=fr, converged=converged, records=records, stats=fr.explore_stats)


def final(run):
    """What tells two runs apart at the end: rule count, the last episode's steps, the consequents' bytes."""
    fr = run["fr"]
    return (fr.five.R, fr.ep_steps, np.array(fr.five.rconc[: fr.five.R]).tobytes())
