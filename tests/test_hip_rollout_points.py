"""Roll-outs that keep every agent's visited-point set (frirl_hip_rollout_points, csrc/rollout_points.hip) and the map-preserving
reduction of a whole batch built on them (frirl_hip_batch_reduce_all_map, frirl_demo --reduce-map).

The rule bases are those of tests/test_hip_reduce_batch.py (trained by the oracle, trig_mode = 1), the start rows those of
tests/test_hip_rollout_batch.py: starts_for (spread_starts).  Point lists are compared as SORTED ROW SETS, bit-wise: the order of a list
is unspecified.

Device against device (points against frirl_hip_rollout_record + frirl_hip_log_points at the same forced rule slices, row outputs
against frirl_hip_rollout_batch's tiled form) needs no margin: both sides run the same shared_sweep instantiation on the same inputs.

Margin condition (tests/test_hip_policy_map.py: check_margin).  Where a set is compared with the ORACLE's episodes, the reference's own
evaluations at every compared point are first shown to leave a relative gap >= 1e-6 between the two best conclusions and no tie.  The
agents and starts were chosen on the CPU so that the reference alone meets it: over the five starts_for rows of every agent of
case(env) the smallest gaps are 6.9e-4 (mountaincar), 4.0e-3 (acrobot) and 1.7e-3 (cartpole), no ties; no case is left out.

1. equal to record + log_points, to rollout_batch and to the oracle   5. overflow, every table size, a full table
2. every lane shape, a run-time Shepard power                         6. reproducible
3. several workgroups per agent                                       7. the order does not matter downstream
4. exploration                                                        8. the batch object, 9. the command line"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import policy_map_ref as ref
from tests.test_hip_policy_map import check_margin
from tests.test_hip_reduce_batch import Trained, agent_for, case, spread_starts, upload
from tests.test_hip_rollout_batch import BASE, SEED, oracle_rows, same_bits, starts_for, tens

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
CAP = frirl_amd.POINTS_MAX_CAP
N = 5
EPS = 0.3
# the two rule bases of a call (indices into case(env)); a third agent, a copy of the first, is skipped.  mountaincar's agent 2 has a
# row whose episode fails (by the oracle alone: test_the_reference_rows_are_the_known_ones)
PAIR = {"mountaincar": (2, 3), "acrobot": (0, 1), "cartpole": (0, 1)}
ROW_COUNT = [N, 2, N]


def row_set(points):
    """the rows of [k][ns] float64 as a sorted list of their bytes"""
    return sorted(np.ascontiguousarray(r, dtype=np.float64).tobytes() for r in points)


def mix(env, skipped="inactive"):
    """(Problem of three agents, starts [3 * N][ns], active or None): case(env)[PAIR[0]], case(env)[PAIR[1]] and a copy of the first that
    is skipped -- inactive, or with a rule count of 0 / maxR + 1"""
    a, b = (case(env)[i] for i in PAIR[env])
    prob = upload([a, b, a])[0]
    all_starts = starts_for(env, N)
    starts = np.concatenate([all_starts[i * N:(i + 1) * N] for i in PAIR[env] + (PAIR[env][0],)])
    active = None
    if skipped == "inactive":
        active = tens(np.array([1, 1, 0], np.uint8))
    else:
        prob.nrules[2] = 0 if skipped == "no rules" else prob.maxR + 1
    return prob, np.ascontiguousarray(starts), active


def points_call(prob, agent, n, starts, cap=CAP, only_successful=False, row_count=None, active=None):
    """One call into sentinel-filled buffers with one more agent's block of sentinel behind `points`: host (points [E][cap][ns], count,
    overflow, steps, reward, success) after checking that nothing was written at or beyond point_count[e] or behind the array."""
    import torch
    E, ns = prob.E, prob.nant - 1
    whole = torch.full((E + 1, cap, ns), SENT, dtype=torch.float64, device=DEV)
    count = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    over = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    s = None if starts is None else tens(np.ascontiguousarray(starts).reshape(E * n, ns))
    out = prob.rollout_points(agent, n, cap=cap, only_successful=only_successful, start_states=s, row_count=row_count, active=active,
                              out=(whole[:E], count, over))
    torch.cuda.synchronize()
    pts, count, over = whole.cpu().numpy(), count.cpu().numpy(), over.cpu().numpy()
    assert (pts[E] == SENT).all(), "written behind the array"
    for e in range(E):
        assert 0 <= count[e] <= cap and over[e] in (0, 1), (e, count[e], over[e])
        assert (pts[e, count[e]:] == SENT).all(), (e, "rows at or beyond point_count were written")
        assert len(set(row_set(pts[e, : count[e]]))) == count[e], (e, "a point is listed twice")
    return (pts[:E], count, over) + tuple(x.cpu().numpy() for x in out[3:])


def record_points(prob, agent, n, starts, only_successful=False, row_count=None, active=None, cap=1024):
    """frirl_hip_rollout_record (one episode per log, T = max_steps + 1) -> frirl_hip_log_points with a cap no set reaches: host (list of
    [count][ns] arrays, ep_steps, ep_reward, ep_success)"""
    import torch
    E, ns = prob.E, prob.nant - 1
    s = None if starts is None else tens(np.ascontiguousarray(starts).reshape(E * n, 1, ns))
    log = prob.rollout_record(agent, n, 1, agent.desc.max_steps + 1, start_states=s, row_count=row_count, active=active)
    pts, count, over = log.points(cap, only_successful)
    torch.cuda.synchronize()
    assert (over.cpu().numpy() == 0).all()
    pts, count = pts.cpu().numpy(), count.cpu().numpy()
    return [pts[e, : count[e]] for e in range(E)], log.ep_steps[:, 0].cpu().numpy(), log.ep_reward[:, 0].cpu().numpy(), log.ep_success[:, 0].cpu().numpy()


def assert_same_sets(got, want, where):
    pts, count, over = got[:3]
    for e, w in enumerate(want):
        assert over[e] == 0 and count[e] == len(w), (where, e, int(count[e]), len(w), int(over[e]))
        assert row_set(pts[e, : count[e]]) == row_set(w), (where, e)


def slices(hip_option, H):
    hip_option("rollout_points_slices", H)
    hip_option("rollout_record_slices", H)


@functools.lru_cache(maxsize=None)
def oracle_sets(env, e):
    """By the oracle alone, for agent e of case(env) and its N starts_for rows: (per-row de-duplicated points, success flags, Diag of
    the reference's evaluation at every one of these points)"""
    a = case(env)[e]
    a.restore(a.rant, a.rconc)
    ms = frirl_amd.demo_describe(env)["max_steps"]
    ave = np.array(a.fr.action_vevalues)
    starts = starts_for(env, N)[e * N:(e + 1) * N]
    diag = ref.Diag()
    rows, ok = [], []
    for x0 in starts:
        pts = ref.episode_points(a.fr, x0, ms)
        rows.append(ref.dedup(pts))
        for pt in rows[-1]:
            ref.evaluate(a.fr.five, pt, ave, diag)
    a.fr.set_start_state(a.start)
    return rows, oracle_rows(env, N)[3][e * N:(e + 1) * N], diag


# ---- 1. against record + log_points, rollout_batch and the oracle ---------------------------------------------------------------
def test_the_reference_rows_are_the_known_ones():
    """By the oracle alone: what the cases below rely on."""
    mc = oracle_rows("mountaincar", N)
    assert mc[1][2 * N:3 * N].tolist() == [409, 261, 255, 1000, 269] and mc[3][2 * N:3 * N].tolist() == [1, 1, 1, 0, 1]
    assert oracle_rows("acrobot", N)[3].all() and oracle_rows("acrobot", N)[1].max() <= 185
    assert oracle_rows("cartpole", N)[3].tolist() == [0] * 9 + [1], "cartpole: nine of ten rows contribute nothing with only_successful"
    for env in ("mountaincar", "acrobot", "cartpole"):
        rows, ok, diag = oracle_sets(env, PAIR[env][0])
        check_margin(diag)
        assert 20 < len(ref.dedup(np.concatenate(rows))) < 200


@pytest.mark.parametrize("only_successful", [False, True])
@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_sets_equal_record_and_log_points(env, only_successful, hip_option):
    hip_option("rollout_batch_resident", 0)
    prob, starts, active = mix(env)
    agent = agent_for(env)
    rc = tens(np.array(ROW_COUNT, np.int32))
    for H in (0, 4):
        slices(hip_option, H)
        got = points_call(prob, agent, N, starts, only_successful=only_successful, row_count=rc, active=active)
        want, ep_steps, ep_reward, ep_success = record_points(prob, agent, N, starts, only_successful, rc, active)
        print(env, only_successful, H, "points", got[1], "steps", got[3])
        assert_same_sets(got, want, (env, H))
        assert got[1][2] == 0 and got[2][2] == 0, "a skipped agent: no point, no overflow"
        assert (got[3] == ep_steps).all() and (got[5] == ep_success).all() and same_bits(got[4], ep_reward)
        steps, reward, success, _ = (x.cpu().numpy() for x in prob.rollout_batch(agent, N, start_states=tens(starts), row_count=rc, active=active))
        assert (got[3] == steps).all() and (got[5] == success).all() and same_bits(got[4], reward), "bit for bit the rows of rollout_batch"
        assert (steps[N + 2:2 * N] == -1).all() and (steps[2 * N:] == -1).all() and (steps[:N + 2] >= 0).all()
    if only_successful:
        full = points_call(prob, agent, N, starts, row_count=rc, active=active)
        assert (got[1] <= full[1]).all()
        for e in range(2):
            assert set(row_set(got[0][e, : got[1][e]])) <= set(row_set(full[0][e, : full[1][e]]))
        if env == "mountaincar":
            assert got[1][0] < full[1][0], "the failing row contributed points of its own"
        if env == "cartpole":
            assert got[1][0] == 0 and full[1][0] > 0, "no successful row: no point"
    # one agent against the oracle: the union of its rows' episode points
    rows, ok, diag = oracle_sets(env, PAIR[env][0])
    check_margin(diag)
    keep = [r for r, s in zip(rows, ok) if s == 1 or not only_successful]
    want0 = ref.dedup(np.concatenate(keep)) if keep else np.zeros((0, prob.nant - 1))
    assert got[1][0] == len(want0) and row_set(got[0][0, : got[1][0]]) == row_set(want0), "agent 0: the oracle's points"


@pytest.mark.parametrize("skipped", ["no rules", "too many rules"])
def test_agents_with_a_bad_rule_count_are_skipped(skipped):
    env = "mountaincar"
    prob, starts, active = mix(env, skipped)
    assert active is None
    agent = agent_for(env)
    got = points_call(prob, agent, N, starts)
    want = record_points(prob, agent, N, starts)
    assert_same_sets(got, want[0], skipped)
    assert got[1][2] == 0 and got[2][2] == 0 and got[1][0] > 0 and (got[3][2 * N:] == -1).all() and (got[4][2 * N:] == 0).all() and (got[5][2 * N:] == 0).all()
    assert (got[3] == want[1]).all() and same_bits(got[4], want[2]) and (got[5] == want[3]).all()


def test_max_steps_zero_keeps_the_start_states():
    """max_steps = 0: the reference's episode (policy_map_ref.episode_points, range(max_steps)) asks the policy at the un-quantised start
    and nowhere else; the row ends on the iteration that began it.  An agent's set is the set of its rows' start states."""
    env, n = "mountaincar", 3
    agents = case(env)[:2]
    starts = starts_for(env, n)[:2 * n]
    agent = agent_for(env)
    agent.desc.max_steps = 0
    got = points_call(upload(agents)[0], agent, n, starts)
    want = []
    for e, a in enumerate(agents):
        a.restore(a.rant, a.rconc)
        rows = [ref.episode_points(a.fr, x0, 0) for x0 in starts[e * n:(e + 1) * n]]
        assert all(same_bits(r, x0[None]) for r, x0 in zip(rows, starts[e * n:(e + 1) * n]))
        want.append(ref.dedup(np.concatenate(rows)))
    assert [len(w) for w in want] == [n, n], "the start rows differ"
    assert_same_sets(got, want, "max_steps = 0")
    assert (got[3] == 0).all() and (got[4] == 0.0).all() and (got[5] == 0).all() and len(got[3]) == 2 * n


# ---- 2. lane shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_every_lane_shape(env, hip_option):
    prob, starts, active = mix(env)
    agent = agent_for(env)
    first = None
    for H in (1, 4, 8):
        slices(hip_option, H)
        got = points_call(prob, agent, N, starts, active=active)
        want = record_points(prob, agent, N, starts, active=active)
        assert_same_sets(got, want[0], (env, H))
        assert (got[3] == want[1]).all() and same_bits(got[4], want[2])
        sets = [row_set(w) for w in want[0]]
        if first is None:
            first = sets, want[1]
        assert sets == first[0] and (want[1] == first[1]).all(), (H, "the recorded roll-outs agree across rule slices at the default power")
        assert [row_set(got[0][e, : got[1][e]]) for e in range(3)] == first[0], (H, "so do the point sets")
    # n = 1: a full wave per row; NULL start states = agent.values_def
    slices(hip_option, 0)
    a0 = case(env)[PAIR[env][0]]
    agent1 = agent_for(env, a0.start)
    got = points_call(prob, agent1, 1, None, active=active)
    want = record_points(prob, agent1, 1, None, active=active)
    assert_same_sets(got, want[0], (env, "n = 1"))
    rows, _, diag = oracle_sets(env, PAIR[env][0])
    check_margin(diag)
    assert row_set(got[0][0, : got[1][0]]) == row_set(rows[0]), "row 0 of starts_for is the agent's own start: the oracle's episode from it"
    # a run-time Shepard power
    agent2 = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV, p=2)
    for H in (0, 8):
        slices(hip_option, H)
        got = points_call(prob, agent2, N, starts, active=active)
        want = record_points(prob, agent2, N, starts, active=active)
        assert_same_sets(got, want[0], (env, "p = 2", H))
        assert (got[3] == want[1]).all() and same_bits(got[4], want[2]) and (got[5] == want[3]).all()


# ---- 3. several workgroups per agent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("only_successful", [False, True])
def test_several_workgroups_per_agent(only_successful, hip_option):
    """E = 2, n = 70: with 4 lanes per row and 8 / 4 / 1 rule slices a workgroup serves 8 / 16 / 64 rows, so an agent has 9 / 5 / 2
    workgroups, the last one partly filled; the finalise launch merges their segments."""
    env, n = "mountaincar", 70
    agents = [case(env)[2], case(env)[3]]
    prob = upload(agents)[0]
    starts = np.concatenate([spread_starts(a.fr, n, 0.15, seed=70 + e) for e, a in enumerate(agents)])
    agent = agent_for(env)
    rc = tens(np.array([n, 37], np.int32))
    for H in (8, 4, 1):
        slices(hip_option, H)
        got = points_call(prob, agent, n, starts, only_successful=only_successful, row_count=rc)
        want = record_points(prob, agent, n, starts, only_successful, rc)
        assert_same_sets(got, want[0], (H, only_successful))
        assert (got[3] == want[1]).all() and same_bits(got[4], want[2]) and (got[5] == want[3]).all()
        assert (got[3][n + 37:] == -1).all() and (got[3][:n + 37] >= 0).all()
        print(H, "points", got[1], "successes", int(got[5].sum()))
    assert got[1].min() > 40, "more points than one row visits"
    assert 0 < got[5].sum() < n + 37, "some rows fail, some succeed"


# ---- 4. exploration ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "cartpole"])
def test_exploring_rollouts(env, hip_option):
    prob, starts, active = mix(env)
    d = frirl_amd.demo_describe(env)
    agent = frirl_amd.demo_agent(d, DEV, epsilon=EPS, no_random=0, seed=SEED, env_id_base=BASE)
    greedy = points_call(prob, agent_for(env), N, starts, active=active)
    for H in (0, 1):
        slices(hip_option, H)
        got = points_call(prob, agent, N, starts, active=active)
        want = record_points(prob, agent, N, starts, active=active)
        assert_same_sets(got, want[0], (env, "exploring", H))
        assert (got[3] == want[1]).all() and same_bits(got[4], want[2]) and (got[5] == want[3]).all()
    assert (got[3] != greedy[3]).any(), "exploration was meant to change rows"


# ---- 5. overflow ------------------------------------------------------------------------------------------------------------------
def test_overflow():
    """cap = 8 on acrobot: agent 0's five rows visit 87 points.  Agent 1 has one row, from a start beside the goal: by the oracle its
    episode takes 8 steps over 6 distinct points."""
    env = "acrobot"
    prob, starts, active = mix(env)
    starts = starts.copy()
    starts[N] = (3.1, 0.0, 0.0, 0.0)
    a1 = case(env)[PAIR[env][1]]
    a1.restore(a1.rant, a1.rconc)
    by_oracle = ref.dedup(ref.episode_points(a1.fr, starts[N], 1000))
    assert len(by_oracle) == 6
    agent = agent_for(env)
    rc = tens(np.array([N, 1, N], np.int32))
    full = points_call(prob, agent, N, starts, row_count=rc, active=active)
    got = points_call(prob, agent, N, starts, cap=8, row_count=rc, active=active)
    assert full[2].tolist() == [0, 0, 0] and full[1][0] > 8 and full[1][1] <= 8
    assert got[2].tolist() == [1, 0, 0] and got[1].tolist() == [8, full[1][1], 0]
    kept = row_set(got[0][0, :8])
    assert len(set(kept)) == 8 and set(kept) <= set(row_set(full[0][0, : full[1][0]])), "eight distinct members of the whole set"
    assert row_set(got[0][1, : got[1][1]]) == row_set(full[0][1, : full[1][1]]) == row_set(by_oracle)
    assert (got[3] == full[3]).all() and same_bits(got[4], full[4]), "the rows do not depend on cap"
    # cap = exactly the set's size: no overflow
    exact = points_call(prob, agent, N, starts, cap=int(full[1][0]), row_count=rc, active=active)
    assert exact[2].tolist() == [0, 0, 0] and exact[1][0] == full[1][0]
    less = points_call(prob, agent, N, starts, cap=int(full[1][0]) - 1, row_count=rc, active=active)
    assert less[2].tolist() == [1, 0, 0] and less[1][0] == full[1][0] - 1


def test_table_sizes_and_a_full_table(hip_option):
    """The LDS table has 256 / 512 / 768 slots for cap <= 128 / 384 / 512 and takes 128 entries fewer.  Acrobot agent 3 visits more than
    128 points from five starts (136 by the oracle with these), agent 0 fewer: every cap on either side of a threshold gives the whole
    set or a subset of cap members with the overflow flag; with one workgroup per agent (rule slices 1) and cap = 100 the 256-slot
    table itself fills up (128 entries) before the rows have ended."""
    env = "acrobot"
    agents = [case(env)[3], case(env)[0]]
    prob = upload(agents)[0]
    all_starts = starts_for(env, N, seed0=50)
    starts = np.concatenate([all_starts[3 * N:4 * N], all_starts[:N]])
    agent = agent_for(env)
    full = points_call(prob, agent, N, starts)
    want = record_points(prob, agent, N, starts)
    assert_same_sets(full, want[0], "cap 512")
    sets = [set(row_set(full[0][e, : full[1][e]])) for e in range(2)]
    print("points", full[1])
    assert full[1][0] > 128 > full[1][1] > 100
    for H in (0, 1):
        slices(hip_option, H)
        for cap in (100, 128, 129, 384, 385):
            got = points_call(prob, agent, N, starts, cap=cap)
            for e in range(2):
                fits = full[1][e] <= cap
                assert got[2][e] == (0 if fits else 1) and got[1][e] == (full[1][e] if fits else cap), (H, cap, e, got[1], got[2])
                mine = set(row_set(got[0][e, : got[1][e]]))
                assert mine == sets[e] if fits else mine < sets[e], (H, cap, e)
            assert (got[3] == full[3]).all() and same_bits(got[4], full[4])


# ---- 6. reproducible --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,n", [("mountaincar", 70), ("acrobot", N)])
def test_two_identical_calls_return_identical_arrays(env, n):
    agents = [case(env)[i] for i in PAIR[env]]
    prob = upload(agents)[0]
    starts = np.concatenate([spread_starts(a.fr, n, 0.15 if env == "mountaincar" else 0.05, seed=70 + e) for e, a in enumerate(agents)])
    agent = agent_for(env)
    one = points_call(prob, agent, n, starts, only_successful=True)
    two = points_call(prob, agent, n, starts, only_successful=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two)), "order included"
    assert one[1].min() > 0


# ---- 7. the order does not matter downstream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_reduction_from_points_equals_reduction_from_logs(env):
    import torch
    agents = [case(env)[i] for i in PAIR[env]]
    agent = agent_for(env)
    starts = np.concatenate([starts_for(env, N)[i * N:(i + 1) * N] for i in PAIR[env]])
    state = []
    for source in ("points", "logs"):
        prob, rant_d, _ = upload(agents, with_uidx=True)
        if source == "points":
            pts, count, over = prob.rollout_points(agent, N, start_states=tens(starts))[:3]
        else:
            log = prob.rollout_record(agent, N, 1, agent.desc.max_steps + 1, start_states=tens(starts.reshape(2 * N, 1, -1)))
            pts, count, over = log.points(CAP)
        best0, _ = prob.policy_map(agent, pts, point_count=count, actconc=False)
        res, kept = prob.reduce_batch_map(agent, pts, point_count=count, strategy=1, rant=rant_d)
        best1, _ = prob.policy_map(agent, pts, point_count=count, actconc=False)
        torch.cuda.synchronize()
        assert (over.cpu().numpy() == 0).all()
        assert (best0.cpu().numpy() == best1.cpu().numpy()).all(), "the reduced rule base's map is the un-reduced one's at every point"
        state.append(([k.tolist() for k in kept], [(r.rules_before, r.rules_after, r.points) for r in res], prob.rb.cpu().numpy(), prob.nrules.cpu().numpy(),
                      rant_d.cpu().numpy(), prob.uidx.cpu().numpy()))
    a, b = state
    assert a[0] == b[0] and a[1] == b[1], "the same rules survive"
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:])), "the same device state"
    assert any(r[1] < r[0] for r in a[1]), "something was removed"


# ---- 8. the batch object ----------------------------------------------------------------------------------------------------------
def rulebase_of(b, e, nant, maxR):
    R = C.c_int32()
    rant, rconc = np.zeros((maxR, nant)), np.zeros(maxR)
    DP = C.POINTER(C.c_double)
    frirl_amd.check(frirl_amd.lib().frirl_hip_batch_get_rulebase(b, e, C.byref(R), rant.ctypes.data_as(DP), rconc.ctypes.data_as(DP)), "frirl_hip_batch_get_rulebase")
    return R.value, rant[: R.value].copy(), rconc[: R.value].copy()


@pytest.mark.parametrize("only_successful", [True, False])
def test_batch_reduce_all_map(only_successful):
    """Four mountain-car agents trained on the device for at most 39 episodes (by the oracle: all four then solve most of their rows,
    not all), reduced by frirl_hip_batch_reduce_all_map and by hand on a copy of their rule bases."""
    import torch
    env, E, n, maxR, nant = "mountaincar", 4, 4, 512, 3
    L = frirl_amd.lib()
    probe = ob.Frirl(env, trig_mode=1)
    own = spread_starts(probe, E, 0.15)
    rows = np.stack([spread_starts(probe, n, 0.15, seed=60 + e) for e in range(E)])
    rows[:, 0] = own
    b = frirl_amd.demo_batch_object(env, E, maxR, start_states=own)
    try:
        eps = C.c_int32(-1)
        frirl_amd.check(L.frirl_hip_batch_train(b, 40, C.byref(eps)), "frirl_hip_batch_train")
        tot = frirl_amd.ReduceMapTotals()
        for bad in (dict(n=0), dict(n=257), dict(strategy=0), dict(strategy=3), dict(cap=-1), dict(cap=513), dict(n=2, starts=None)):
            kw = dict(dict(strategy=1, n=n, starts=rows.ctypes.data_as(C.POINTER(C.c_double)), cap=0), **bad)
            assert L.frirl_hip_batch_reduce_all_map(b, kw["strategy"], kw["n"], kw["starts"], 1, kw["cap"], None, C.byref(tot)) == -2, bad
            assert b"frirl_hip_batch_reduce_all_map" in L.frirl_hip_last_error()
        before = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        # the manual pipeline on a copy: the oracle snaps the device's rules into its tables (Trained asserts that they come back bit-equal)
        agents = [Trained(env, own[e], rules=(before[e][1], before[e][2])) for e in range(E)]
        prob, rant_d, _ = upload(agents, with_uidx=True, maxR=maxR)
        agent = agent_for(env)
        starts = tens(rows.reshape(E * n, nant - 1))
        steps0, reward0, success0, _ = (x.cpu().numpy() for x in prob.rollout_batch(agent, n, start_states=starts))
        pts, count, over = prob.rollout_points(agent, n, only_successful=only_successful, start_states=starts)[:3]
        res_m, kept = prob.reduce_batch_map(agent, pts, point_count=count, active=(over == 0).to(torch.uint8), strategy=1, rant=rant_d)
        steps1, reward1, success1, _ = (x.cpu().numpy() for x in prob.rollout_batch(agent, n, start_states=starts))
        torch.cuda.synchronize()
        count, over = count.cpu().numpy(), over.cpu().numpy()
        print("steps", steps0, "success", success0, "points", count, "rules", [(r.rules_before, r.rules_after) for r in res_m])
        # the call
        res, tot = frirl_amd.batch_reduce_all_map(b, 1, n, rows, only_successful=only_successful)
        after = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        nr, rb, ra = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), rant_d.cpu().numpy()
        for e in range(E):
            assert (res[e].rules_before, res[e].rules_after, res[e].points, res[e].tries) == (res_m[e].rules_before, res_m[e].rules_after, res_m[e].points, res_m[e].tries), e
            R = int(nr[e])
            assert after[e][0] == R == res[e].rules_after and res[e].rules_before == before[e][0], e
            assert same_bits(after[e][1], np.ascontiguousarray(ra[e, :, :R].T)) and same_bits(after[e][2], rb[e, nant, :R]), e
            assert same_bits(after[e][1], before[e][1][kept[e]]) and same_bits(after[e][2], before[e][2][kept[e]]), (e, "the surviving rules, in order")
        assert (over == 0).all()
        assert tot.agents_reduced == sum(r.rules_after < r.rules_before for r in res) and tot.agents_overflow == 0
        assert tot.agents_without_points == int((count == 0).sum()) and tot.points == int(count.sum()) == sum(r.points for r in res)
        assert tot.rules_before == sum(r.rules_before for r in res) and tot.rules_after == sum(r.rules_after for r in res)
        assert tot.points > 0 and tot.agents_reduced > 0, "the agents were meant to solve some of their rows, and to lose rules"
        # greedy episodes from the starts that contributed are reproduced: steps and reward bits
        sel = (success0 == 1) | (not only_successful)
        assert sel.any() and (steps1[sel] == steps0[sel]).all() and (success1[sel] == success0[sel]).all() and same_bits(reward1[sel], reward0[sel])
        # every agent's own start (NULL, n = 1), cap 1: everything overflows, nothing changes
        res1, tot1 = frirl_amd.batch_reduce_all_map(b, 1, 1, None, only_successful=False, cap=1)
        assert tot1.agents_overflow == E and tot1.agents_reduced == 0 and tot1.points == 0 and tot1.rules_after == tot1.rules_before == tot.rules_after
        assert all(r.rules_after == r.rules_before and r.tries == 0 for r in res1)
        again = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        assert all(x[0] == y[0] and same_bits(x[1], y[1]) and same_bits(x[2], y[2]) for x, y in zip(after, again))
        # the batch goes on learning
        assert L.frirl_hip_batch_train(b, 3, C.byref(eps)) == 0, L.frirl_hip_last_error()
    finally:
        L.frirl_hip_batch_destroy(b)


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------
def test_demo_reduce_map(tmp_path):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    base = [demo, "--env", "mountaincar", "--agents", "4", "--reduce", "1", "--reduce-all"]
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path)
    mapped = subprocess.run(base + ["--reduce-map", "4"], capture_output=True, text=True, cwd=tmp_path)
    every = subprocess.run(base + ["--reduce-map", "4", "--reduce-map-all", "--spread", "0.1"], capture_output=True, text=True, cwd=tmp_path)
    assert plain.returncode == 0 and mapped.returncode == 0 and every.returncode == 0, (plain.stderr, mapped.stderr, every.stderr)
    assert "reduced-map:" not in plain.stdout and os.path.exists(tmp_path / "mountaincar.batch.reduced1.frirlrb.txt")
    p, m = plain.stdout.splitlines(), mapped.stdout.splitlines()
    assert len(p) == 2 and " agents reduced, " in p[1], plain.stdout
    assert len(m) == 2 and m[0] == p[0] and m[1].startswith("reduced-map: batch mountaincar: "), mapped.stdout
    assert "successful starts" in m[1] and "all starts" in every.stdout.splitlines()[1]
    words = m[1].replace(",", " ").split()
    reduced, before, after = int(words[3]), int(words[8]), int(words[10])
    assert 0 < reduced <= 4 and 0 < after < before, m[1]
    assert int(words[words.index("overflow") + 1]) == 0 and int(words[words.index("points") + 1]) > 0
    out = tmp_path / "mountaincar.batch.reducedmap1.frirlrb.txt"
    assert out.exists() and out.stat().st_size > 0
