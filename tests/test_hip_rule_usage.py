"""Rule usage on the policy map and the stable rule order on the device (frirl_hip_rule_usage, frirl_hip_rule_order;
csrc/rule_usage.hip) against the CPU reference over the oracle (tests/rule_usage_ref.py: the oracle's FIVE_vag_concl_weight at every
point and its greedy action).

Inputs: map_case of tests/test_hip_policy_map.py (E = 3 agents with 70 / 0 / 37 points, every fourth point an exact hit, every fourth a
duplicate, U = 41) at p = 0 and 3 over a covering subset of (nant, A, R): R = 300 crosses one 256-rule block of the second launch,
A = 21 / 32 with 70 points crosses one pass of points of the first.  The margin condition of that file is asserted first: the greedy
action decides WHICH action's weights are summed.  Tolerance: the project's Q tolerance, 1e-9 relative."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from tests import policy_map_ref as pm
from tests import rule_usage_ref as ref
from tests.problems import Batch
from tests.test_hip_policy_map import COUNTS, E_MAP, N_MAP, U, check_margin, map_case, synth_agent, tens
from tests.test_hip_reduce_batch import SENTINEL, device

pytestmark = pytest.mark.gpu

USAGE_CASES = [(2, 1, 1), (2, 3, 300), (3, 21, 300), (3, 32, 2), (5, 1, 65), (5, 21, 65), (5, 32, 300), (8, 3, 65), (8, 32, 300)]


def close(got, want):
    return bool((np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-300).all())


def usage_into(prob, agent, points, count, active, total, peak, best):
    """frirl_hip_rule_usage into the caller's arrays (Problem.rule_usage allocates zeroed ones)"""
    L = frirl_amd.lib()
    mp = prob._map_points(points, count, active)
    out = frirl_amd.RuleUsageOut(total.data_ptr(), peak.data_ptr() if peak is not None else None, best.data_ptr() if best is not None else None)
    nbytes = L.frirl_hip_rule_usage_workspace_bytes(prob.nant, prob.E, mp.n)
    import torch
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=points.device)
    frirl_amd.check(L.frirl_hip_rule_usage(C.byref(prob.tables), C.byref(prob._bases), C.byref(agent.desc), C.byref(mp), C.byref(out), ws.data_ptr(), nbytes,
                                           frirl_amd._stream()), "frirl_hip_rule_usage")
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0, 3])
@pytest.mark.parametrize("nant,A,R", USAGE_CASES)
def test_usage_matches_reference(nant, A, R, p):
    import torch
    b, ave, avals, pts, _, diag = map_case(nant, A, R, p)
    check_margin(diag)
    want = [ref.usage(b.five(e, p), pts[e, : COUNTS[e]], ave) for e in range(E_MAP)]
    prob = b.to_device(device())
    maxR = prob.maxR
    agent = synth_agent(b, ave, avals, p)
    points, count = tens(pts), tens(np.array(COUNTS, dtype=np.int32))
    mk = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=device())
    total, peak, best = mk((E_MAP, maxR), SENTINEL, torch.float64), mk((E_MAP, maxR), SENTINEL, torch.float64), mk((E_MAP, N_MAP), -7, torch.int32)
    usage_into(prob, agent, points, count, None, total, peak, best)
    map_best, _ = prob.policy_map(agent, points, point_count=count, actconc=False)
    torch.cuda.synchronize()
    total_h, peak_h, best_h = total.cpu().numpy(), peak.cpu().numpy(), best.cpu().numpy()
    assert (best_h == map_best.cpu().numpy()).all(), "best is frirl_hip_policy_map's, -1 for points that do not exist"
    for e in range(E_MAP):
        n = COUNTS[e]
        ws, wp, wb = want[e]
        assert (best_h[e, :n] == wb).all() and (best_h[e, n:] == -1).all()
        assert close(total_h[e, :R], ws) and close(peak_h[e, :R], wp), (e, np.abs(total_h[e, :R] - ws).max())
        assert abs(total_h[e, :R].sum() - n) <= 1e-9 * n, "every point hands out weights that sum to 1"
        assert (total_h[e, R:] == 0).all() and (peak_h[e, R:] == 0).all(), "zeros in [R, maxR)"
        if n == 0:
            assert (total_h[e] == 0).all() and (peak_h[e] == 0).all(), "no point: zeros"
        else:
            assert (peak_h[e, :R] <= total_h[e, :R]).all() and (peak_h[e, :R] <= 1.0).all() and (peak_h[e, :R] >= 0).all()
    # other agents switched off: their rows keep the sentinel, best reads -1; the remaining agent has the same bits; without peak / best
    active = tens(np.array([0, 0, 1], dtype=np.uint8))
    total2, peak2, best2 = mk((E_MAP, maxR), SENTINEL, torch.float64), mk((E_MAP, maxR), SENTINEL, torch.float64), mk((E_MAP, N_MAP), -7, torch.int32)
    usage_into(prob, agent, points, count, active, total2, peak2, best2)
    total3 = mk((E_MAP, maxR), SENTINEL, torch.float64)
    usage_into(prob, agent, points, count, active, total3, None, None)
    total2, peak2, best2, total3 = total2.cpu().numpy(), peak2.cpu().numpy(), best2.cpu().numpy(), total3.cpu().numpy()
    assert (total2[:2] == SENTINEL).all() and (peak2[:2] == SENTINEL).all() and (best2[:2] == -1).all()
    assert total2[2].tobytes() == total_h[2].tobytes() == total3[2].tobytes() and peak2[2].tobytes() == peak_h[2].tobytes() and (best2[2] == best_h[2]).all()
    # the wrapper: zeroed rows for agents that are skipped
    s, pk, bb = prob.rule_usage(agent, points, point_count=count, active=active, peak=True)
    torch.cuda.synchronize()
    assert s.cpu().numpy()[2].tobytes() == total_h[2].tobytes() and (s.cpu().numpy()[:2] == 0).all() and pk.cpu().numpy()[2].tobytes() == peak_h[2].tobytes()
    assert (bb.cpu().numpy() == best2).all()


def test_usage_does_not_depend_on_the_launch_shape(hip_option):
    """rules in LDS or in global memory, one action per lane or blocks of four, an agent alone or among others, more points allocated
    than exist: the same bits; a rule count outside 1..maxR leaves the rows alone"""
    import torch
    nant, A, R, p = 5, 3, 300, 0
    b, ave, avals, pts, _, _ = map_case(nant, A, R, p)
    prob = b.to_device(device())
    agent = synth_agent(b, ave, avals, p)
    count = tens(np.array(COUNTS, dtype=np.int32))
    wide = tens(np.concatenate([pts, pts], axis=1))                       # n = 140: 140 * 3 > 256, blocks of four actions
    out = {}
    for resident in (1, 0):
        hip_option("reduce_map_resident", resident)
        out[resident] = prob.rule_usage(agent, tens(pts), point_count=count, peak=True)
        out[resident, "wide"] = prob.rule_usage(agent, wide, point_count=count, peak=True)
    torch.cuda.synchronize()
    s0, p0, b0 = (x.cpu().numpy() for x in out[1])
    for key, (s, pk, bb) in out.items():
        assert s.cpu().numpy().tobytes() == s0.tobytes() and pk.cpu().numpy().tobytes() == p0.tobytes(), key
        assert (bb.cpu().numpy()[:, :N_MAP] == b0).all() and (bb.cpu().numpy()[:, N_MAP:] == -1).all(), key
    prob.nrules[0] = 0
    prob.nrules[2] = b.maxR + 1
    s, _, bb = prob.rule_usage(agent, tens(pts), point_count=count)
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0).all() and (bb.cpu().numpy() == -1).all(), "agents 0 and 2 skipped (the wrapper's zeros), agent 1 has no point"


def test_rule_order_by_consequent_on_ragged_rule_counts():
    """keys = NULL: the candidate order of strategy 1 / 2, ties by index; rule counts 300, 7, 0 (skipped), and others; inactive rows untouched"""
    import torch
    nant, R, E = 3, 300, 5
    b = Batch(nant, U, R, E, A=3, seed=9, ragged=True)
    assert b.nrules[0] == R and b.nrules[1] == 7 and b.nrules[2] == 0
    q = b.rb[:, nant, :]
    q[0, 20], q[0, 200], q[0, 299], q[3, 1] = -q[0, 10], q[0, 10], -q[0, 10], q[3, 0]      # |Q| ties, across a block of 256
    prob = b.to_device(device())
    active = tens(np.array([1, 1, 1, 1, 0], dtype=np.uint8))
    for descending in (False, True):
        order = torch.full((E, b.maxR), -9, dtype=torch.int32, device=device())
        prob.rule_order(None, descending=descending, active=active, out=order)
        torch.cuda.synchronize()
        order = order.cpu().numpy()
        for e in range(E):
            n = int(b.nrules[e]) if e != 4 else 0
            assert list(order[e, :n]) == pm.candidate_order(q[e, :n], 2 if descending else 1), (e, descending)
            assert (order[e, n:] == -9).all(), "entries at and beyond nrules, and the rows of skipped agents, are untouched"
    full = prob.rule_order(None).cpu().numpy()
    assert list(full[4, : b.nrules[4]]) == pm.candidate_order(q[4, : b.nrules[4]], 1) and (full[2] == -1).all()


@pytest.mark.parametrize("R", [300, 1100])
def test_rule_order_by_keys_with_ties_and_nans(R):
    """the caller's keys: few distinct values, signed zeros, infinities and NaNs; R = 1100 crosses one tile of 1024 staged keys"""
    import torch
    nant, E = 2, 3
    b = Batch(nant, U, R, E, A=3, seed=4, ragged=False)
    prob = b.to_device(device())
    rng = np.random.default_rng(R)
    pool = np.array([0.0, -0.0, 0.25, 0.5, 1.0, -1.0, 3.5, np.inf, -np.inf, np.nan])
    keys = pool[rng.integers(0, len(pool), size=(E, b.maxR))]
    keys[1] = rng.random(b.maxR)
    keys[1, 5], keys[1, R - 1] = np.nan, np.nan
    keys_d = tens(keys)
    for descending in (False, True):
        order = prob.rule_order(keys_d, descending=descending)
        torch.cuda.synchronize()
        order = order.cpu().numpy()
        for e in range(E):
            want = ref.stable_order(keys[e, :R], descending)
            assert list(order[e, :R]) == want, (e, descending)
            assert np.isnan(keys[e, want[-1]]) and (order[e, R:] == -1).all()
