"""The policy map, the reduction validated on it and the points of recorded roll-outs on the device (frirl_hip_policy_map,
frirl_hip_reduce_batch_map, frirl_hip_log_points; csrc/policy_map.hip, csrc/reduce_map_kernels.h) against the CPU reference over the
oracle (tests/policy_map_ref.py).

Margin condition.  Device and oracle Q agree to about 1e-11 (tests/test_hip_q.py), so a greedy action -- and with it a try-remove
decision -- can differ from the reference's only where the two best conclusions are closer than that.  Every test that compares greedy
actions therefore first asserts, on the REFERENCE's own evaluations of its inputs, that the smallest relative gap between the two best
conclusions is >= 1e-6 (the project's contract on interpolated Q, five orders above the observed agreement) and that no two best
conclusions are bit-equal unless both are exact hits.  The inputs were chosen on the CPU so that the reference alone meets both:
  map      MAP_CASES covers every pair (nant, A) of the issue's values and every R with each of them at least once; it is a covering
           subset, not the full 4 x 4 x 4 product.  One-rule bases are paired with A = 1 only: with one rule every action's conclusion
           is that rule's consequent up to the rounding of (w * Q) / w, so the first maximum over several actions is decided by a last
           bit, which nobody promises.  Points at which the reference's own gap is below 1e-5 are drawn again on the CPU
           (map_case): at nant = 8 with the default power 8 and 21 / 32 closely spaced actions the nearest rule dominates every
           conclusion, and the first draw left gaps of 8.1e-9 / 1.3e-9 there.  Every case asserts the margin and compares best exactly.
  reduce   the points are those of ONE greedy episode of the oracle-trained demo rule base.  From the default start the reference's
           smallest gap is 7.8e-7 (mountaincar, strategy 2) and 2.8e-7 / 3.4e-7 (acrobot), so these two episodes start elsewhere
           (POINT_START): mountaincar at position values_def + 0.02 * span; acrobot at values_def + (0.30, 0.30, 0, -0.20) * span.
           cartpole keeps its default start.  The reference's smallest gaps over the agents of a call are then 5.5e-4 / 2.3e-6
           (mountaincar, strategy 1 / 2), 2.6e-6 / 2.5e-6 (acrobot) and 1.3e-5 / 2.9e-6 (cartpole), no ties."""
import functools

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import policy_map_ref as ref
from tests.problems import Batch
from tests.test_hip_reduce_batch import SENTINEL, Trained, agent_for, device, upload

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-6
REDRAW_GAP = 1e-5         # input selection (map_case): ten times the asserted margin
U = 41
E_MAP, N_MAP = 3, 70
COUNTS = [70, 0, 37]
# nant x A, every R: one-rule bases with A = 1 only (see above)
MAP_CASES = [(2, 1, 1), (3, 1, 2), (5, 1, 65), (8, 1, 300), (5, 1, 1), (8, 1, 1),
             (2, 3, 300), (3, 3, 65), (5, 3, 2), (8, 3, 65),
             (2, 21, 2), (3, 21, 300), (5, 21, 65), (8, 21, 2),
             (2, 32, 65), (3, 32, 2), (5, 32, 300), (8, 32, 300)]

def tens(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def check_margin(diag):
    assert diag.evaluations > 0
    assert diag.ties == 0, f"{diag.ties} bit-equal ties between the two best conclusions in the reference's own evaluations"
    assert diag.min_rel_gap >= MIN_GAP, f"reference's smallest relative gap {diag.min_rel_gap} < {MIN_GAP}"


@functools.lru_cache(maxsize=None)
def map_case(nant, A, R, p):
    """E_MAP synthetic rule bases of R rules on shared tables, N_MAP points per agent: every fourth an existing rule's antecedents
    (exact hits for the actions that rule base holds there), every fourth a copy of an earlier point, the others off the grid; the
    reference's map of the existing points and its diagnostics."""
    b = Batch(nant, U, R, E_MAP, A=A, seed=100 * nant + A + R, ragged=False)
    ave, avals = b.action_ve()
    rng = np.random.default_rng(7 * nant + A)
    ns = nant - 1
    lo, hi = b.u[:ns, 0], b.u[:ns, U - 2]
    pts = lo + (hi - lo) * rng.random((E_MAP, N_MAP, ns))
    for e in range(E_MAP):
        for j in range(0, N_MAP, 4):
            r = int(rng.integers(0, R))
            pts[e, j] = b.u[np.arange(ns), b.uidx[e, :ns, r]]
        for j in range(3, N_MAP, 4):
            pts[e, j] = pts[e, j - 3 if j % 8 == 3 else j - 2]
    # Points at which the reference's own two best conclusions are closer than REDRAW_GAP (or tie without both being exact hits) are
    # drawn again, in order and from a generator of their own, keeping their kind; a copy follows its source.  Decided by the oracle
    # alone, on the CPU, before anything runs on the device.
    redraw = np.random.default_rng(1000 + 7 * nant + A)
    fives = [b.five(e, p) for e in range(E_MAP)]
    for e in range(E_MAP):
        for j in range(COUNTS[e]):
            for _ in range(400):
                if j % 4 == 3:
                    pts[e, j] = pts[e, j - 3 if j % 8 == 3 else j - 2]
                d = ref.Diag()
                ref.evaluate(fives[e], pts[e, j], ave, d)
                if d.ties == 0 and d.min_rel_gap >= REDRAW_GAP:
                    break
                assert j % 4 != 3, "a copy of an accepted point"
                if j % 4 == 0:
                    pts[e, j] = b.u[np.arange(ns), b.uidx[e, :ns, int(redraw.integers(0, R))]]
                else:
                    pts[e, j] = lo + (hi - lo) * redraw.random(ns)
            else:
                raise AssertionError(f"no point with a reference gap >= {REDRAW_GAP} found for agent {e}, point {j}")
    diag = ref.Diag()
    want = []
    for e in range(E_MAP):
        want.append(ref.policy_map(fives[e], pts[e, : COUNTS[e]], ave, diag) if COUNTS[e] else None)
    return b, ave, avals, pts, want, diag


def synth_agent(b, ave, avals, p):
    nant = b.nant
    grids = [[0.0, 1.0]] * (nant - 1) + [list(avals)]
    return frirl_amd.Agent(device(), nant, grids, [1.0] * nant, [0.0] * nant, ave, 0.5, 0.9, 1.0, -1.0, p=p, env_kind=frirl_amd.ENV_EXTERNAL)


def close(got, want):
    """1e-9 relative: the tolerance of the project's Q tests"""
    return bool((np.abs(got - want) <= 1e-9 * np.abs(want)).all())


@pytest.mark.parametrize("p", [0, 3])
@pytest.mark.parametrize("nant,A,R", MAP_CASES)
def test_map_matches_reference_and_get_best_action(nant, A, R, p):
    import torch
    b, ave, avals, pts, want, diag = map_case(nant, A, R, p)
    check_margin(diag)
    prob = b.to_device(device())
    agent = synth_agent(b, ave, avals, p)
    points = tens(pts)
    count = tens(np.array(COUNTS, dtype=np.int32))
    best = torch.full((E_MAP, N_MAP), -7, dtype=torch.int32, device=device())
    conc = torch.full((E_MAP, N_MAP, A), SENTINEL, dtype=torch.float64, device=device())
    prob.policy_map(agent, points, point_count=count, out=(best, conc))
    # frirl_hip_get_best_action per agent: one state per agent and call
    ave_d = tens(ave)
    gba = [prob.get_best_action(points[:, j, :].contiguous(), ave_d, p=p) for j in range(N_MAP)]
    torch.cuda.synchronize()
    best, conc = best.cpu().numpy(), conc.cpu().numpy()
    for e in range(E_MAP):
        n = COUNTS[e]
        assert (best[e, n:] == -1).all() and (conc[e, n:] == SENTINEL).all(), "points that do not exist: -1, conclusions untouched"
        if n == 0:
            continue
        wb, wc = want[e]
        assert (best[e, :n] == wb).all(), (e, np.nonzero(best[e, :n] != wb))
        assert close(conc[e, :n], wc)
        assert (best[e, :n] == np.argmax(conc[e, :n], axis=1)).all(), "the first maximum of the device's own conclusions"
        for j in range(n):
            gc, gb = gba[j]
            assert int(gb[e]) == best[e, j] and close(conc[e, j], gc[e].cpu().numpy())
    # an inactive agent; without conclusions; bits do not depend on the other agents' presence
    active = tens(np.array([0, 1, 1], dtype=np.uint8))
    best2 = torch.full((E_MAP, N_MAP), -7, dtype=torch.int32, device=device())
    conc2 = torch.full((E_MAP, N_MAP, A), SENTINEL, dtype=torch.float64, device=device())
    prob.policy_map(agent, points, point_count=count, active=active, out=(best2, conc2))
    best3, none = prob.policy_map(agent, points, actconc=False)
    torch.cuda.synchronize()
    best2, conc2, best3 = best2.cpu().numpy(), conc2.cpu().numpy(), best3.cpu().numpy()
    assert none is None
    assert (best2[0] == -1).all() and (conc2[0] == SENTINEL).all()
    assert (best2[1:] == best[1:]).all() and (conc2[1:] == conc[1:]).all()
    assert (best3[0] == best[0]).all() and (best3[2, : COUNTS[2]] == best[2, : COUNTS[2]]).all() and (best3 >= 0).all()


def test_map_forms_give_the_same_bits(hip_option):
    """rules staged in LDS or read from global memory, one action per lane (n * A <= 256) or blocks of four, points alone or among
    others: the conclusions are bit-equal.  A rule count outside 1..maxR reads -1."""
    import torch
    nant, A, R, p = 5, 3, 300, 0
    b, ave, avals, pts, _, _ = map_case(nant, A, R, p)
    prob = b.to_device(device())
    agent = synth_agent(b, ave, avals, p)
    points = tens(pts)
    out = {}
    for resident in (1, 0):
        hip_option("reduce_map_resident", resident)
        out[resident] = prob.policy_map(agent, points)                                   # 70 * 3 <= 256: one action per lane
        out[resident, "wide"] = prob.policy_map(agent, tens(np.concatenate([pts, pts], axis=1)))      # 140 * 3 > 256: blocks of four
    torch.cuda.synchronize()
    b0, c0 = (x.cpu().numpy() for x in out[1])
    assert (b0 >= 0).all()
    for key, (bb, cc) in out.items():
        bb, cc = bb.cpu().numpy(), cc.cpu().numpy()
        assert (bb[:, :N_MAP] == b0).all() and (cc[:, :N_MAP] == c0).all(), key
        if bb.shape[1] > N_MAP:
            assert (bb[:, N_MAP:] == b0).all() and (cc[:, N_MAP:] == c0).all(), key
    prob.nrules[1] = 0
    prob.nrules[2] = b.maxR + 1
    bad, _ = prob.policy_map(agent, points)
    torch.cuda.synchronize()
    bad = bad.cpu().numpy()
    assert (bad[0] == b0[0]).all() and (bad[1:] == -1).all()


# ---- reduce -----------------------------------------------------------------------------------------------------------------------
# start of the ONE episode whose points validate the removals, as an offset from values_def in units of each state's span (docstring)
POINT_START = {"mountaincar": (0.02, 0.0), "acrobot": (0.30, 0.30, 0.0, -0.20), "cartpole": (0.0, 0.0, 0.0, 0.0)}


@functools.lru_cache(maxsize=None)
def trained(env):
    """the rule base the oracle learns from the default start, and the start of the episode that gives the points"""
    probe = ob.Frirl(env, trig_mode=1)
    dims = [probe.dim(k) for k in range(probe.nstates)]
    default = np.array([d["values_def"] for d in dims])
    span = np.array([d["values"][-1] - d["values"][0] for d in dims])
    return Trained(env, default), default + np.array(POINT_START[env]) * span


def mix(env):
    """agents of one call: the demo rule base; its first half with about half of the points; the rule base with no point; an inactive
    one; a one-rule base.  Returns (agents, point counts as a function of the number of points P, active flags)."""
    t, _ = trained(env)
    half = Trained(env, t.start, rules=(t.rant[: t.R0 // 2], t.rconc[: t.R0 // 2]))
    one = Trained(env, t.start, rules=(t.rant[:1], t.rconc[:1]))
    return [t, half, t, t, one], (lambda P: [P, P // 2 + 1, 0, P, P]), [1, 1, 1, 0, 1]


@functools.lru_cache(maxsize=None)
def reference(env, strategy, points_key):
    """the reference's reduction of every agent of mix(env) at the given points (a tuple of tuples) and its diagnostics"""
    pts = np.array(points_key).reshape(len(points_key), -1)
    agents, counts, active = mix(env)
    f = agents[0].fr.five
    u, ve, ave = np.array(f.u), np.array(f.ve), np.array(agents[0].fr.action_vevalues)
    diag = ref.Diag()
    outs = []
    for a, n, act in zip(agents, counts(len(pts)), active):
        outs.append(ref.reduce_map(u, ve, a.rant, a.rconc, pts[: n if act else 0], ave, strategy, diag=diag))
    return outs, diag


def episode_points_on_device(env):
    """the points of the episode from POINT_START, through frirl_hip_rollout_record + frirl_hip_log_points on the demo rule base alone"""
    import torch
    t, start = trained(env)
    prob, _, _ = upload([t])
    agent = agent_for(env, start)
    log = prob.rollout_record(agent, 1, 1, agent.desc.max_steps + 1)
    points, count, overflow = log.points(256)
    torch.cuda.synchronize()
    assert int(overflow[0]) == 0
    pts = points[0, : int(count[0])].cpu().numpy()
    t.restore(t.rant, t.rconc)
    want = ref.dedup(ref.episode_points(t.fr, start, agent.desc.max_steps))
    assert pts.shape == want.shape and (pts == want).all(), "the recorded episode's points are those of the oracle's greedy episode"
    return pts


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("strategy", [1, 2])
@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_reduce_matches_reference(env, strategy, resident, hip_option):
    import torch
    pts = episode_points_on_device(env)
    P = len(pts)
    outs, diag = reference(env, strategy, tuple(map(tuple, pts)))
    check_margin(diag)
    agents, counts, active = mix(env)
    counts = counts(P)
    E = len(agents)
    prob, rant_d, (rb_h, rant_h, uidx_h) = upload(agents, with_uidx=True)
    nant, maxR = prob.nant, prob.maxR
    agent = agent_for(env)
    points = tens(np.broadcast_to(pts, (E, P, nant - 1)))
    count_d, active_d = tens(np.array(counts, dtype=np.int32)), tens(np.array(active, dtype=np.uint8))
    hip_option("reduce_map_resident", resident)
    best0, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    res, kept = prob.reduce_batch_map(agent, points, point_count=count_d, active=active_d, strategy=strategy, rant=rant_d)
    best1, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    torch.cuda.synchronize()
    assert (best1.cpu().numpy() == best0.cpu().numpy()).all(), "the reduced rule bases' map is the un-reduced ones' at every point"
    rb, rant, uidx, nrules = prob.rb.cpu().numpy(), rant_d.cpu().numpy(), prob.uidx.cpu().numpy(), prob.nrules.cpu().numpy()
    removed_any = False
    for e, (a, out) in enumerate(zip(agents, outs)):
        untouched = not active[e] or counts[e] == 0 or a.R0 == 1
        r = res[e]
        assert (r.rules_before, r.rules_after, r.points, r.tries) == (a.R0, len(out.kept), counts[e] if active[e] else 0, out.tries), (e, r.rules_after, r.tries)
        assert list(kept[e]) == out.kept and int(nrules[e]) == len(out.kept)
        if untouched:
            assert out.kept == list(range(a.R0)) and r.tries == 0
            assert (rb[e] == rb_h[e]).all() and (rant[e] == rant_h[e]).all() and (uidx[e] == uidx_h[e]).all()
            continue
        assert active[e] and (best0[e, : counts[e]].cpu().numpy() == out.best0).all()
        k = len(out.kept)
        removed_any = removed_any or k < a.R0
        assert (rb[e, :nant, :k] == a.veval[:, out.kept]).all() and (rb[e, nant, :k] == a.rconc[out.kept]).all()
        assert (rant[e, :, :k] == a.rant[out.kept].T).all() and (uidx[e, :, :k] == a.uidx[:, out.kept]).all()
        assert (rb[e, :, k: a.R0] == 0).all() and (rant[e, :, k: a.R0] == 0).all() and (uidx[e, :, k: a.R0] == 0).all(), "vacated tail zeroed"
        assert (rb[e, :, a.R0:] == SENTINEL).all() and (rant[e, :, a.R0:] == SENTINEL).all() and (uidx[e, :, a.R0:] == 3).all()
        assert out.kept == sorted(out.kept) and 1 <= k <= a.R0
    assert removed_any


SYNTH_REDUCE = dict(nant=3, A=21, R=40, n=100, counts=[100, 43], seed=1)


@functools.lru_cache(maxsize=None)
def synth_reduce_case(strategy):
    """Two synthetic rule bases with 21 actions and 100 / 43 off-grid and on-grid points: blocks of four actions, six lanes per point,
    42 points per pass, so a try takes up to three passes and is cut short after the first or second one.  The seed was chosen on the
    CPU so that the reference meets the margin condition for both strategies (smallest gaps 1.8e-4 / 3.5e-5; 34 + 31 and 35 + 32 of
    40 + 40 rules kept)."""
    c = SYNTH_REDUCE
    b = Batch(c["nant"], U, c["R"], 2, A=c["A"], seed=c["seed"], ragged=False)
    ave, avals = b.action_ve()
    ns = c["nant"] - 1
    rng = np.random.default_rng(c["seed"])
    lo, hi = b.u[:ns, 0], b.u[:ns, U - 2]
    pts = lo + (hi - lo) * rng.random((2, c["n"], ns))
    for e in range(2):
        for j in range(0, c["n"], 5):
            pts[e, j] = b.u[np.arange(ns), b.uidx[e, :ns, int(rng.integers(0, c["R"]))]]
    diag = ref.Diag()
    rants = [np.ascontiguousarray(b.u[np.arange(c["nant"])[:, None], b.uidx[e, :, : c["R"]]].T) for e in range(2)]
    outs = [ref.reduce_map(b.u, b.ve, rants[e], np.ascontiguousarray(b.rb[e, c["nant"], : c["R"]]), pts[e, : c["counts"][e]], ave, strategy, diag=diag)
            for e in range(2)]
    return b, ave, avals, pts, outs, diag


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("strategy", [1, 2])
def test_reduce_many_points_in_several_passes(strategy, resident, hip_option):
    import torch
    c = SYNTH_REDUCE
    b, ave, avals, pts, outs, diag = synth_reduce_case(strategy)
    check_margin(diag)
    prob = b.to_device(device(), compressed=True)
    agent = synth_agent(b, ave, avals, 0)
    points, count = tens(pts), tens(np.array(c["counts"], dtype=np.int32))
    hip_option("reduce_map_resident", resident)
    best0, _ = prob.policy_map(agent, points, point_count=count, actconc=False)
    res, kept = prob.reduce_batch_map(agent, points, point_count=count, strategy=strategy)
    best1, _ = prob.policy_map(agent, points, point_count=count, actconc=False)
    torch.cuda.synchronize()
    assert (best1.cpu().numpy() == best0.cpu().numpy()).all()
    rb, uidx, nant = prob.rb.cpu().numpy(), prob.uidx.cpu().numpy(), c["nant"]
    for e, out in enumerate(outs):
        k = len(out.kept)
        assert (res[e].rules_before, res[e].rules_after, res[e].points, res[e].tries) == (c["R"], k, c["counts"][e], out.tries)
        assert list(kept[e]) == out.kept and 1 <= k < c["R"]
        assert (best0[e, : c["counts"][e]].cpu().numpy() == out.best0).all()
        assert (rb[e, :, :k] == b.rb[e][:, out.kept]).all() and (rb[e, :, k:] == 0).all()
        assert (uidx[e, :, :k] == b.uidx[e][:, out.kept]).all() and (uidx[e, :, k:] == 0).all()


def test_reduce_refuses_a_bad_rule_count():
    import torch
    t, _ = trained("mountaincar")
    prob, rant_d, (rb_h, _, _) = upload([t, t])
    prob.nrules[1] = 0
    pts = tens(np.zeros((2, 4, 2)))
    with pytest.raises(frirl_amd.FrirlHipError, match="agent 1: nrules outside"):
        prob.reduce_batch_map(agent_for("mountaincar"), pts)
    torch.cuda.synchronize()
    assert int(prob.nrules[0]) == t.R0 and (prob.rb.cpu().numpy()[0] == rb_h[0]).all(), "nothing reduced"
    # the same agent inactive: fine, and left alone
    res, kept = prob.reduce_batch_map(agent_for("mountaincar"), pts, active=tens(np.array([1, 0], dtype=np.uint8)))
    assert (res[1].rules_before, res[1].rules_after, res[1].points, res[1].tries) == (0, 0, 0, 0) and res[0].rules_before == t.R0


# ---- log_points -------------------------------------------------------------------------------------------------------------------
def hand_made_logs():
    """2 agents x 3 logs, T = 12, two episodes per log: a point repeated inside an episode, across episodes and across logs, a start
    state equal to a quantised observation elsewhere, an unsuccessful episode, a log that is cut short, -0.0 beside 0.0."""
    E, n_logs, T, ns = 2, 3, 12, 2
    Q = E * n_logs
    rng = np.random.default_rng(3)
    obs = rng.random((Q, T, ns)) + 10.0                       # never equal to a q_obs below
    q_obs = np.round(rng.random((Q, T, ns)) * 3) / 2          # few distinct values: many repeats
    success = np.zeros((Q, T), dtype=np.int32)
    start = np.zeros((Q, T), dtype=np.uint8)
    length = np.array([12, 11, 9, 12, 12, 7], dtype=np.int32)
    for q in range(Q):
        second = 4 + q % 3                                     # episodes [0, second) and [second, length)
        start[q, 0] = start[q, second] = 1
        success[q, second - 1] = 1
        success[q, length[q] - 1] = 1
    success[1, length[1] - 1] = 0                              # agent 0, log 1: the second episode fails
    success[4, 4 + 4 % 3 - 1] = 0                              # agent 1, log 1: the first episode fails
    obs[2, 0] = q_obs[0, 3]                                    # a start state that an earlier log saw as a quantised observation
    q_obs[3, 2] = (0.0, 0.5)
    q_obs[3, 3] = (-0.0, 0.5)                                  # bit-wise: not the same point
    q_obs[5, 1] = q_obs[3, 5]                                  # repeated across logs
    return obs, q_obs, success, start, length, E


@pytest.mark.parametrize("only_successful", [False, True])
def test_log_points_equal_the_reference(only_successful):
    import torch
    obs, q_obs, success, start, length, E = hand_made_logs()
    want, over = ref.log_points(obs, q_obs, success, start, length, E, 72, only_successful)
    assert (over == 0).all() and all(6 < len(w) < 36 for w in want)
    if only_successful:
        full, _ = ref.log_points(obs, q_obs, success, start, length, E, 72, False)
        assert all(len(w) < len(f) for w, f in zip(want, full)), "the unsuccessful episodes contributed points of their own"
    args = [tens(x) for x in (obs, q_obs, success, start, length)]
    pts, count, overflow = frirl_amd.log_points(*args, E, 72, only_successful)
    small = min(len(w) for w in want) - 2
    pts_s, count_s, overflow_s = frirl_amd.log_points(*args, E, small, only_successful)
    torch.cuda.synchronize()
    pts, count, overflow = pts.cpu().numpy(), count.cpu().numpy(), overflow.cpu().numpy()
    pts_s, count_s, overflow_s = pts_s.cpu().numpy(), count_s.cpu().numpy(), overflow_s.cpu().numpy()
    for e in range(E):
        n = len(want[e])
        assert count[e] == n and overflow[e] == 0
        assert pts[e, :n].tobytes() == want[e].tobytes(), "bit for bit, first occurrence first"
        assert (pts[e, n:] == 0).all(), "rows behind the list are left as they were"
        assert count_s[e] == small and overflow_s[e] == 1 and pts_s[e].tobytes() == want[e][:small].tobytes()
