"""CPU checks of the exploration reference: tests/explore_ref.py against published SplitMix64 outputs, the oracle's restatement
(orc_rng_unit, orc_e_greedy_pick) against explore_ref bit for bit, and dry runs of the oracle alone on the exploring cases of
tests/test_hip_explore.py and tests/test_hip_external.py, which show that those cases can tell a wrong kernel from a right one."""
import itertools
import struct

import numpy as np
import pytest

from oracle import binding as ob
from tests import explore_cases as xc
from tests import explore_ref as er

GIDS = [0, 1, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 3]
EPISODES = [0, 1, 2 ** 31 - 1]
STEPS = [0, 1, 999, 2 ** 24]
MIN_GAP = 1e-9          # relative gap below which a greedy pick could go either way within the kernels' 1e-6 contract on Q


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_known_answers():
    for keys, want in er.known_answers():
        assert er.word(*keys) == want, keys
        assert ob.rng_word(*keys) == want, keys
        assert er.unit(*keys) == (want >> 11) / 2.0 ** 53
    assert er.c_round(0.5) == 1 and er.c_round(0.49999999999999994) == 0 and er.c_round(2.5) == 3 and er.c_round(31.5) == 32


def test_global_ids_repeat_with_period_2_to_the_32():
    for gid in (0, 5, 77):
        assert er.word(9, gid, 3, 4, 1) == er.word(9, gid + 2 ** 32, 3, 4, 1) == er.word(9, gid + 2 ** 40, 3, 4, 1)
        assert er.word(9, gid, 3, 4, 1) != er.word(9, gid + 1, 3, 4, 1)


def test_oracle_stream_and_pick_equal_the_reference():
    """orc_rng_unit == explore_ref, words as integers and units by their bits, over the key edges 7 ids x 3 episodes x 4 steps x
    2 draws = 168 key tuples for each of 64 seeds (10 752 tuples); orc_e_greedy_pick == explore_ref.pick for A = 1..32 and four
    (epsilon, no_random) pairs at the keys of the first 5 seeds (420 x 32 x 4 = 53 760 picks)."""
    seeds = [0, 1, 1234, 2 ** 63 + 12345, 2 ** 64 - 1] + [er.mix64(i) for i in range(1, 60)]
    n = words = 0
    for seed, gid, ep, step in itertools.product(seeds, GIDS, EPISODES, STEPS):
        for draw in (0, 1):
            w = er.word(seed, gid, ep, step, draw)
            assert ob.rng_word(seed, gid, ep, step, draw) == w, (seed, gid, ep, step, draw)
            assert bits(ob.rng_unit(seed, gid, ep, step, draw)) == bits(er.unit(seed, gid, ep, step, draw))
            assert 0.0 <= er.unit(seed, gid, ep, step, draw) < 1.0
            words += 1
        for A in (range(1, 33) if seed in seeds[:5] else ()):
            greedy = (A * 7 + step) % A
            for eps, nr in ((0.3, 0), (1.0, 0), (0.0, 0), (0.7, 1)):
                want = er.pick(greedy, A, eps, nr, seed, gid, ep, step)
                assert ob.e_greedy_pick(greedy, A, eps, nr, seed, gid, ep, step) == want, (A, eps, nr, seed, gid, ep, step)
                assert 0 <= want < A
                n += 1
    assert words >= 10000 and n >= 10000, (words, n)


def test_reduction_replays_stay_greedy():
    """orc_reduce_run forces no_random = 1 for its replays, as the device's reduction does, and restores the agent's setting."""
    a, b = xc.trained("mountaincar"), xc.trained("mountaincar")
    b.set_exploration(0.5, 0, 99, 3)
    assert a.reduce(1, 0.0) == b.reduce(1, 0.0)
    assert (np.array(a.five.rconc[: a.five.R]) == np.array(b.five.rconc[: b.five.R])).all()
    b.episode_eval()
    assert b.explore_stats["explored"] > 0, "exploration is on again after the reduction"


def test_default_oracle_never_consults_the_stream():
    fr = ob.Frirl("mountaincar", trig_mode=1)
    for _ in range(3):
        fr.episode()
    st = fr.explore_stats
    assert st["picks"] > 0 and st["explored"] == 0 and fr.rng_episode == 3


@pytest.mark.parametrize("env", xc.DEMOS)
def test_demo_cases_explore_enough_and_have_no_near_ties(env):
    """The oracle alone on the committed seeds: every case has at least 10 exploring picks that change the action, and no pick that
    stayed greedy has its two best conclusions within 1e-9 relative unless they are bit-equal (the all-zero initial rule base, where
    both sides take the first maximum) -- so the comparisons with the device need no tie allowance.  At least 8 roll-out rows outlive
    the staged roll-out's cap.  The printed figures are recorded in profiles/r09_explore_parity.md."""
    _, stats = xc.learning_case(env)
    cons = [c["stats"] for c in xc.construct_case(env)]
    for name, sts in (("learning", stats), ("construct", cons)):
        changed, clamped = sum(s["changed"] for s in sts), sum(s["clamped"] for s in sts)
        gap = np.nanmin([s["min_gap"] for s in sts])
        print(f"{env} {name}: picks {sum(s['picks'] for s in sts)} exploring {sum(s['explored'] for s in sts)} changed {changed} clamped {clamped} "
              f"smallest greedy gap {gap:.3e}")
        assert changed >= 10 and gap >= MIN_GAP, (name, changed, gap)
        assert all(s["changed"] >= 1 for s in sts), "every environment's own stream matters"
    for masked in (False, True):
        rc = xc.rollout_case(env, masked)
        sts = rc["stats"]
        changed, clamped = sum(s["changed"] for s in sts), sum(s["clamped"] for s in sts)
        gap = np.nanmin([s["min_gap"] for s in sts])
        parked = int((rc["steps"] > xc.ROLLOUT_CAP).sum())
        print(f"{env} roll-outs masked={masked}: picks {sum(s['picks'] for s in sts)} changed {changed} clamped {clamped} smallest greedy gap {gap:.3e} "
              f"parked rows {parked} of {xc.Q}")
        assert changed >= 10 and gap >= MIN_GAP and parked >= 8, (masked, changed, gap, parked)
    plain, masked = xc.rollout_case(env, False), xc.rollout_case(env, True)
    differ = (plain["steps"] != masked["steps"]) | (plain["reward"] != masked["reward"])
    assert not differ[0::4].any() and (differ.any() or env == "mountaincar"), "mask 0 changes nothing; the others are exercised"


@pytest.mark.parametrize("nant", [2, 5, 8])
@pytest.mark.parametrize("A", [3, 11])
def test_new_shape_cases_explore_enough(nant, A):
    """The exploring new-shape cases of tests/test_hip_external.py, the mirrors alone: at least 10 exploring picks that change the
    action per case, and few near-ties among the picks that stayed greedy (the tie rule allows 10 % of those)."""
    from tests.test_hip_external import EXPLORE, new_shape_case
    d, env, starts, mirrors = new_shape_case(nant, A, explore=EXPLORE)
    for _ in range(4):
        for m in mirrors:
            if not m.converged:
                m.episode(env, None)
    picks, near = sum(m.picks for m in mirrors), sum(m.near for m in mirrors)
    changed, clamped = sum(m.changed for m in mirrors), sum(m.clamped for m in mirrors)
    print(f"nant {nant} A {A}: picks {picks} exploring {sum(m.explored for m in mirrors)} changed {changed} clamped {clamped} near-ties {near}")
    assert changed >= 10 and near * 10 <= picks - sum(m.explored for m in mirrors), (picks, near, changed)
