"""CPU side of the hyper-parameter tests (no GPU): the oracle's treatment of alpha, gamma, the qdiff bounds, weight_significant and
skip_rules against runs of the genuine reference with the same overrides (fixtures tests/golden/hparams/, written by
oracle/make_golden.py through ref_harness' demo_hp mode), and the conditions under which the device cases of
tests/test_hip_hparams.py mean something, each asserted on the oracle alone: a non-default set changes the result (a kernel that
ignored the field would fail), the branches the sets are meant to reach are reached, the greedy picks of the admitted trajectory
cases keep a margin, and the caller-stepped cases stay under the near-tie cap.
"""
import json
import os

import numpy as np
import pytest

from oracle import binding as ob
from tests import hparams_cases as hc


def load_jsonl(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


# ---- 1. the oracle against the genuine reference ---------------------------------------------------------------------------------
def test_set_hparams_reaches_the_agent():
    fr = ob.Frirl("acrobot")
    before = fr.hparams
    fr.set_hparams(alpha=0.25, weight_thr=0.002, skip_rules=0)
    after = fr.hparams
    assert (after["alpha"], after["weight_thr"], after["skip_rules"]) == (0.25, 0.002, 0)
    assert all(after[k] == before[k] for k in before if k not in ("alpha", "weight_thr", "skip_rules"))
    a = fr.agent()
    assert (a.alpha, a.gamma, a.qdiff_pos, a.qdiff_neg, a.weight_thr, a.skip_rules) == tuple(after[k] for k in hc.HP_KEYS)
    assert (a.c.alpha, a.c.weight_significant, a.c.skip_rules) == (0.25, 0.002, 0)
    with pytest.raises(AssertionError):
        fr.set_hparams(weight=0.1)


@pytest.mark.parametrize("env,name,nep", hc.REF_CASES)
def test_oracle_matches_the_reference_off_the_demos_values(env, name, nep, golden_dir, tmp_path):
    """As tests/test_oracle_golden.py::test_demo_matches_reference_run, for runs of the reference whose frirl_desc had its SARSA
    hyper-parameters overridden (libm trig on both sides): per episode steps, reward bits, rule count and the running hash over every
    action / state / reward / quantised state / rule count of every step; then the rule base text.  skip_rules = 0 (update_rules' other
    variant, frirl_update_sarsa.c:45-73) on every demo, the thresholds 0.002 and 0.3 on one demo each."""
    tr = load_jsonl(os.path.join(golden_dir, "hparams", f"{env}_{name}.trace.jsonl"))
    eps = [r for r in tr if r["k"] == "ep"]
    end = [r for r in tr if r["k"] == "end"][0]
    assert len(eps) == nep == end["episodes"]
    fr = hc.demo_frirl(env, name, trig_mode=0)
    for rec in eps:
        fr.episode()
        assert fr.ep_steps == rec["steps"], rec["ep"]
        assert fr.ep_reward == float.fromhex(rec["reward"]), rec["ep"]
        assert fr.five.R == rec["R"], rec["ep"]
        assert "%016x" % fr.step_hash == rec["hash"], rec["ep"]
    assert (fr.total_steps, fr.five.R, "%016x" % fr.step_hash) == (end["total_steps"], end["R"], end["hash"])
    p = str(tmp_path / "rb.txt")
    fr.save_text(p)
    with open(p) as a, open(os.path.join(golden_dir, "hparams", f"{env}_{name}.frirlrb.txt")) as b:
        assert a.read() == b.read(), "rule base differs from the reference's"
    # the override is not a no-op: the demo's own values give another run
    own = ob.Frirl(env)
    for _ in range(nep):
        own.episode()
    assert own.step_hash != fr.step_hash


# ---- 2. whole trajectories: margins, sensitivity, branches -----------------------------------------------------------------------
def trajectory_differs(a, b):
    fa, fb = a["fr"].five, b["fr"].five
    return fa.R != fb.R or a["total_steps"] != b["total_steps"] or (np.array(fa.rconc[: fa.R]) != np.array(fb.rconc[: fb.R])).any()


@pytest.mark.parametrize("env,name", hc.TRAJ_CASES)
def test_trajectory_cases_are_admitted(env, name):
    """Per admitted case the oracle's own run (portable trig, maxR 512, max_episodes 14 / 8 / 6 for mountaincar / acrobot / cartpole)
    keeps min_gap >= 1e-6 at every greedy pick, stays within 135 rules and 10 000 steps, and differs from the default set's run.
    Measured (min_gap, rules, total steps; most / fewest rules one spread wrote):
      mountaincar thr_small               2.48e-06  106  9720   17 / 0
      mountaincar noskip_thr_small_tight  3.21e-06   97  8568    4 / 2
      acrobot     noskip                  5.37e-05   38  1539   11 / 0
      acrobot     thr0                    1.06e-06   34  1186   34 / 32
      acrobot     thr_big                 9.10e-05  135   947    2 / 0
      acrobot     alpha_gamma             1.11e-04   46  2763   11 / 0
      acrobot     never_insert            1.38e-05   32   741   16 / 0
      cartpole    noskip                  3.29e-06   70   700   12 / 0
      cartpole    thr_small               1.29e-05   43   103   32 / 1
      cartpole    thr_big                 1.26e-02   46    89    2 / 0
      cartpole    noskip_thr_small_tight  3.32e-05   43   108   33 / 1
      cartpole    alpha_gamma             3.04e-05   55   180   14 / 0
    Not admitted at these lengths: mountaincar noskip 3.4e-07, thr0 6.5e-10, thr_big 1.3e-07, alpha_gamma 1.4e-16 and never_insert
    (neither reaches the goal: 13 000 steps); acrobot thr_small and the combined set 1.1e-16; cartpole thr0 4.5e-09, never_insert
    2.1e-06 (admissible but thin; acrobot carries that set)."""
    r = hc.traj_run(env, name)
    print(env, name, "min_gap %.3g" % r["stats"]["min_gap"], "rules", r["fr"].five.R, "steps", r["total_steps"], r["spread"])
    assert r["stats"]["min_gap"] >= hc.MIN_GAP, r["stats"]
    assert r["stats"]["explored"] == 0 and r["stats"]["picks"] > r["total_steps"]
    assert r["fr"].five.R <= 135 and r["total_steps"] <= 10000 and r["converged"] == 0
    assert trajectory_differs(r, hc.traj_run(env, "default")), "the set changes nothing on this demo"


def test_every_set_is_admitted_somewhere_and_reaches_its_branches():
    sets = {name for _, name in hc.TRAJ_CASES}
    assert sets == set(hc.NON_DEFAULT)
    runs = {(env, name): hc.traj_run(env, name) for env, name in hc.TRAJ_CASES}
    for name in ("thr0", "thr_small"):          # more than the 19 rules a threshold of 0.05 allows
        assert max(r["spread"]["moved_max"] for (_, n), r in runs.items() if n == name) > 19, name
    assert min(r["spread"]["moved_min"] for (_, n), r in runs.items() if n == "thr_big") == 0, "a spread that writes no rule"
    for (env, n), r in runs.items():
        if n == "thr0":          # walking every rule in every spread is more work than the snapped-point sweeps of the out-of-bounds updates
            assert r["spread"]["spread_rules"] > r["spread"]["outside_rules"] > 0, r["spread"]
        if n == "never_insert":
            assert r["fr"].five.R == 2 ** r["fr"].nant and r["spread"]["spreads"] > 0


# ---- 3. update level ---------------------------------------------------------------------------------------------------------------
def update_signature(c):
    return [(r["status"], r["fus"].tobytes(), [q.tobytes() for q in r["rconc"]]) for r in c.rounds]


@pytest.mark.parametrize("E", [96, 256])
@pytest.mark.parametrize("table", range(len(hc.UPDATE_TABLES)), ids=hc.UPDATE_TABLE_IDS)
def test_update_cases_reach_their_branches(table, E):
    """The eight rounds of every update-level case on the oracle: every non-default set changes some environment's status or
    consequents; EXACT and SPREAD are seen in every case, INSERTED unless never_insert (whose rule count never changes), SKIPPED exactly
    under skip_rules = 1; the crafted rounds find environments with the sticky flag set and take the branches they are built for.
    Under thr0, thr_small and the combined set some spread writes more than 19 rules (at point2x3 every rule there is: its rule grid
    has 15 places), under thr_big some spread writes none.  Measured, most rules one spread wrote at E = 96 / 256 (tables of 84, 62,
    54, 6 and 275 rules: mountaincar, cartpole, acrobot, point 2 x 3, point 8 x 3): thr0 87/88, 67/66, 59/59, 11/10, 280/280;
    thr_small 86/87, 65/66, 57/55, 11/10, 56/68; combined set 86/87, 65/66, 56/55, 11/10, 42/53; thr_big 3, 2, 2, 2, 2 at most and 0
    at least on every table; the default set 9/10, 9/9, 9/9, 6/8, 8/8."""
    base = hc.update_case(table, "default", E)
    small_table = base.table.R < 20
    for name in hc.SETS:
        c = hc.update_case(table, name, E)
        print(hc.UPDATE_TABLE_IDS[table], name, E, "R0", c.table.R, "moved", c.moved_min, c.moved_max, sorted(c.seen))
        if name != "default":
            assert update_signature(c) != update_signature(base), name
        want = {hc.EXACT, hc.SPREAD} | ({hc.INSERTED} if name != "never_insert" else set()) | ({hc.SKIPPED} if c.h["skip_rules"] == 1 else set())
        assert c.seen == want, (name, c.seen)
        if name == "never_insert":
            assert all((r["R"] == c.table.R).all() for r in c.rounds)
        for rnd in (hc.ROUNDS, hc.ROUNDS + 1):
            r = c.rounds[rnd]
            assert r["crafted"].sum() >= E // 8, (name, rnd)
            inside = rnd == hc.ROUNDS or name == "never_insert"
            expect = hc.SKIPPED if inside and c.h["skip_rules"] == 1 else hc.EXACT
            assert all(r["status"][e] == expect for e in np.nonzero(r["crafted"])[0]), (name, rnd)
        if name in ("thr0", "thr_small", "noskip_thr_small_tight"):
            assert c.moved_max > (c.table.R if small_table else 19), (name, c.moved_max)
        if name == "thr_big":
            assert c.moved_min == 0 and c.moved_max <= 3


# ---- 4c. caller-stepped agents on the point shapes ---------------------------------------------------------------------------------
def dry_run(nant, A, name):
    from tests.test_hip_external import new_shape_case, point_desc
    d, env, starts, mirrors = new_shape_case(nant, A, override=hc.overrides(name, point_desc(nant, A), point=True))
    for _ in range(4):
        for m in mirrors:
            if not m.converged:
                m.episode(env, None)
    return mirrors


@pytest.mark.parametrize("nant,A", hc.EXTERNAL_SHAPES)
def test_caller_stepped_cases_stay_under_the_near_tie_cap(nant, A):
    """A dry run of the mirrors of tests/test_hip_external.py (the oracle alone, 16 agents, 4 episodes) per shape and set: picks at
    which the oracle's two best conclusions lie within 1e-12 relative are at most a tenth of the picks (the cap on picks that may
    follow the device), and every set ends with other rule bases than the default.  At 8 x 3 (256 corner rules: more than two rules
    per lane of a 64-lane sweep) thr0 and thr_small write more than two rules of one lane's stride in one spread.
    Measured near-ties / picks:          4 x 5        5 x 11       8 x 3
      default                            38 / 2397    41 / 2504    35 / 2524
      noskip                             39 / 2263    50 / 2567    33 / 2539
      thr0                               35 / 2225    34 / 2463    48 / 2505
      thr_small                          52 / 2391    53 / 2542    70 / 2536
      thr_big                            35 / 2366    36 / 2515    32 / 2511
      noskip_thr_small_tight             75 / 2292    59 / 2529    76 / 2509
      alpha_gamma                        38 / 2337    41 / 2533    33 / 2540
      never_insert                       47 / 2218    32 / 2508    39 / 2406
    (at most 3.3 %).  Rule counts end between 16 and 56, 32 and 82, 256 and 323."""
    base = None
    for name in hc.SETS:
        mirrors = dry_run(nant, A, name)
        near, picks = sum(m.near for m in mirrors), sum(m.picks for m in mirrors)
        st = [m.five.spread_stats for m in mirrors]
        print(nant, A, name, "near", near, "picks", picks, "rules", min(m.five.R for m in mirrors), max(m.five.R for m in mirrors),
              "moved_max", max(x["moved_max"] for x in st), "lane_max", max(x["lane_max"] for x in st))
        assert near * 10 <= picks, (name, near, picks)
        sig = [(m.five.R, np.array(m.five.rconc[: m.five.R]).tobytes()) for m in mirrors]
        if name == "default":
            base = sig
        else:
            assert sig != base, name
        if name in ("thr0", "thr_small"):
            assert max(x["moved_max"] for x in st) > 19, name
            if nant == 8:
                assert max(x["lane_max"] for x in st) > 2, name
        if name == "thr_big":
            assert min(x["moved_min"] for x in st) == 0
        if name == "never_insert":
            assert all(m.five.R == 2 ** nant for m in mirrors)


# ---- 4d. demonstration replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nant,A", hc.TEACH_SHAPES)
def test_replay_cases_depend_on_the_set(nant, A):
    """The replay of tests/teach_ref.py::point_case on the oracle's mirrors: the logs are the scripted teacher's whatever the set, the
    rule bases learned from them differ from the default set's for every set used on the device, skip_rules = 0 never skips and
    skip_rules = 1 does."""
    from tests import teach_ref as tr
    base = None
    for name in ["default"] + hc.TEACH_SETS:
        d, log = tr.point_case(nant, A, hparams=name)
        assert all(d[k] == hc.point_desc(nant, A, name)[k] for k in hc.HP_KEYS)
        mirrors = tr.mirrors_for(d, log, 512)
        for e, m in enumerate(mirrors):
            m.replay(log, e)
        sig = [(m.five.R, np.array(m.five.rconc[: m.five.R]).tobytes()) for m in mirrors]
        skipped = sum(m.branches[tr.SKIPPED] for m in mirrors)
        print(nant, A, name, "rules", [m.five.R for m in mirrors], "skipped", skipped, "spread", sum(m.branches[tr.SPREAD] for m in mirrors))
        if name == "default":
            base = sig
        else:
            assert sig != base, name
        assert (skipped > 0) == (d["skip_rules"] == 1), (name, skipped)
        assert sum(m.branches[tr.SPREAD] for m in mirrors) > 0 and sum(m.branches[tr.EXACT] for m in mirrors) > 0


# ---- 4e. merge -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nant", [3, 5])
def test_merge_cases_depend_on_the_threshold(nant):
    from tests.test_hip_power import merge_case
    out = {}
    for thr in (0.05, 0.002, 0.3):
        b, grids, hp, oag, srant, srconc, spread, fives = merge_case(nant, 0, weight_thr=thr)
        for f in fives:
            f.merge_rb(oag, srant, srconc)
        out[thr] = [np.array(f.rconc[: f.R]).tobytes() for f in fives]
    assert out[0.002] != out[0.05] and out[0.3] != out[0.05]
