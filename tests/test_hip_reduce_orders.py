"""The map-validated reduction over several caller orders on the device (frirl_hip_reduce_batch_map_orders, frirl_hip_rule_order,
frirl_hip_rule_usage, frirl_hip_batch_reduce_all_map_orders; csrc/reduce_orders_kernels.h, csrc/rule_usage.hip) against the CPU
reference over the oracle (tests/rule_usage_ref.py).

Inputs: those of tests/test_hip_policy_map.py::test_reduce_matches_reference (mix(env) at the points of the POINT_START episode, three
demos) and SYNTH_REDUCE.  Per agent K = 4 orders: |Q| ascending, reversed index, default_rng(5).permutation(R), and the REFERENCE's
least-used-first order, computed on the CPU and uploaded.

Margin condition (tests/test_hip_policy_map.py): every comparison of decisions first asserts, on the reference's own evaluations of all
four orders, that the smallest relative gap between the two best conclusions is >= 1e-6 and that there are no ties.

The fourth order.  The orders recorded with this test -- the rule counts of RECORDED and the margins below -- were drawn by handing the
oracle's FIVE_vag_concl_weight the SNAPPED VE values [snapped point, ave[best]], which it snaps a second time as universe values
(tests/rule_usage_ref.py: resnapped).  That is not the usage of the rule base at the point, but here an order is only an INPUT: any
permutation must give the reference's result, so the recorded case is kept as it was recorded (reference's smallest gaps: mountaincar
4.3e-6, acrobot 2.5e-6, cartpole 6.5e-6, synth 1.8e-4 over all four orders, no ties).  The usage the DEVICE computes is the one at
the VE point the map evaluates (include/frirl_hip.h); tests/test_hip_rule_usage.py and the end-to-end test below compare it with the
reference asked at the point itself.  Under THAT least-used-first order the reference keeps 28 / 16 (mountaincar), 99 / 10 (acrobot) and
8 / 6 (cartpole) rules, its usage sums tie for many rules (mountaincar 43 pairs, cartpole 27 / 17: rules that mirror each other about
the greedy action are equally far from every point) and acrobot's smallest decision gap is 7.6e-7, below the 1e-6 margin, so the
end-to-end test compares kept lists exactly only for the agents whose reference sums are apart and whose margin holds (STRICT: how
many of an input's agents that is, decided by the reference alone), and checks the invariants for every agent."""
import ctypes as C
import functools

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import policy_map_ref as pm
from tests import rule_usage_ref as ref
from tests.test_hip_policy_map import SYNTH_REDUCE, check_margin, episode_points_on_device, mix, synth_agent, synth_reduce_case, tens, trained
from tests.test_hip_reduce_batch import SENTINEL, Trained, agent_for, device, spread_starts, upload
from tests.test_hip_rollout_points import rulebase_of, same_bits

pytestmark = pytest.mark.gpu

ENVS = ["mountaincar", "acrobot", "cartpole"]
K = 4
STRICT = {"mountaincar": 1, "acrobot": 1, "cartpole": 0, "synth": 2}
SUM_GAP = 1e-6            # adjacent distinct usage sums of the reference differ by at least this, relatively (end-to-end test)


# rules kept by (reversed, permutation, fourth order) for the demo rule base / its first half: the figures recorded with this test
RECORDED = {"mountaincar": ([28, 29, 34], [18, 16, 16]), "acrobot": ([64, 23, 178], [20, 7, 15]), "cartpole": ([7, 6, 29], [6, 5, 6])}


def four_orders(u, ve, rant, rconc, pts, ave):
    """the K orders of one rule base (module docstring)"""
    R = len(rconc)
    fourth = list(range(R))                                            # an agent that is left alone: its orders are never read
    if R >= 2 and len(pts):
        fourth, _ = ref.usage_order(u, ve, rant, rconc, pts, ave, resnapped=True)
    return [pm.candidate_order(rconc, 1), list(range(R - 1, -1, -1)), [int(r) for r in np.random.default_rng(5).permutation(R)], fourth]


class Case:
    """one agent's reference: orders [K][R], the Outcome of every order, rules kept per order, the chosen k and its Outcome"""

    def __init__(self, u, ve, rant, rconc, pts, ave, diag):
        self.args = (u, ve, rant, rconc, pts, ave)
        self.orders = four_orders(*self.args)
        self.outs = [ref.reduce_map_order(u, ve, rant, rconc, pts, ave, o, diag=diag) for o in self.orders]
        self.after = [len(o.kept) for o in self.outs]
        self.untouched = len(pts) == 0 or len(rconc) < 2
        self.chosen = -1 if self.untouched else int(np.argmin(self.after))
        self.out = self.outs[max(self.chosen, 0)]

    @functools.cached_property
    def by_usage(self):
        """(the reference's usage sums at the points themselves, its least-used-first order, the Outcome under it, that run's Diag)"""
        u, ve, rant, rconc, pts, ave = self.args
        diag = pm.Diag()
        order, total = ref.usage_order(u, ve, rant, rconc, pts, ave, diag=diag)
        return total, order, ref.reduce_map_order(u, ve, rant, rconc, pts, ave, order, diag=diag), diag


@functools.lru_cache(maxsize=None)
def reference(env, points_key):
    pts = np.array(points_key).reshape(len(points_key), -1)
    agents, counts, active = mix(env)
    f = agents[0].fr.five
    u, ve, ave = np.array(f.u), np.array(f.ve), np.array(agents[0].fr.action_vevalues)
    diag = pm.Diag()
    return [Case(u, ve, a.rant, a.rconc, pts[: n if act else 0], ave, diag) for a, n, act in zip(agents, counts(len(pts)), active)], diag


@functools.lru_cache(maxsize=None)
def synth_reference():
    c = SYNTH_REDUCE
    b, ave, avals, pts, _, _ = synth_reduce_case(1)
    diag = pm.Diag()
    rants = [np.ascontiguousarray(b.u[np.arange(c["nant"])[:, None], b.uidx[e, :, : c["R"]]].T) for e in range(2)]
    cases = [Case(b.u, b.ve, rants[e], np.ascontiguousarray(b.rb[e, c["nant"], : c["R"]]), pts[e, : c["counts"][e]], ave, diag) for e in range(2)]
    return b, ave, avals, pts, cases, diag


def orders_tensor(cases, maxR, fill=-7):
    """[E][K][maxR] int32; entries at and beyond R hold `fill`: they are never read"""
    o = np.full((len(cases), K, maxR), fill, dtype=np.int32)
    for e, c in enumerate(cases):
        for k in range(K):
            o[e, k, : len(c.orders[k])] = c.orders[k]
    return o


def sums_are_apart(total):
    """adjacent sums differ by >= SUM_GAP relative, and none tie: the device's order of ITS sums is then the reference's"""
    s = np.sort(total)
    return bool((np.diff(s) >= SUM_GAP * s[1:]).all())


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("env", ENVS)
def test_orders_match_reference(env, resident, hip_option):
    import torch
    pts = episode_points_on_device(env)
    P = len(pts)
    cases, diag = reference(env, tuple(map(tuple, pts)))
    print(env, "min_rel_gap", diag.min_rel_gap, "ties", diag.ties, "after", [c.after for c in cases], "chosen", [c.chosen for c in cases])
    check_margin(diag)
    assert ([c.after[1:] for c in cases[:2]]) == [list(x) for x in RECORDED[env]], "the recorded case"
    agents, counts, active = mix(env)
    counts = counts(P)
    E = len(agents)
    prob, rant_d, (rb_h, rant_h, uidx_h) = upload(agents, with_uidx=True)
    nant, maxR = prob.nant, prob.maxR
    agent = agent_for(env)
    points = tens(np.broadcast_to(pts, (E, P, nant - 1)))
    count_d, active_d = tens(np.array(counts, dtype=np.int32)), tens(np.array(active, dtype=np.uint8))
    orders = tens(orders_tensor(cases, maxR))
    hip_option("reduce_map_resident", resident)
    best0, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    res, kept, after = prob.reduce_batch_map_orders(agent, points, orders, point_count=count_d, active=active_d, rant=rant_d)
    best1, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    torch.cuda.synchronize()
    assert (best1.cpu().numpy() == best0.cpu().numpy()).all(), "the reduced rule bases' map is the un-reduced ones' at every point"
    rb, rant, uidx, nrules = prob.rb.cpu().numpy(), rant_d.cpu().numpy(), prob.uidx.cpu().numpy(), prob.nrules.cpu().numpy()
    removed_any = False
    for e, (a, c) in enumerate(zip(agents, cases)):
        untouched = not active[e] or counts[e] == 0 or a.R0 == 1
        r, out = res[e], c.out
        assert list(after[e]) == c.after, (e, list(after[e]), c.after)
        assert (r.rules_before, r.rules_after, r.points, r.chosen, r.tries) == (a.R0, len(out.kept), counts[e] if active[e] else 0, c.chosen, out.tries if not untouched else 0), e
        assert list(kept[e]) == out.kept and int(nrules[e]) == len(out.kept)
        if untouched:
            assert out.kept == list(range(a.R0)) and r.chosen == -1 and c.after == [a.R0] * K
            assert (rb[e] == rb_h[e]).all() and (rant[e] == rant_h[e]).all() and (uidx[e] == uidx_h[e]).all()
            continue
        assert (best0[e, : counts[e]].cpu().numpy() == out.best0).all()
        assert c.after[c.chosen] == min(c.after) and c.chosen == c.after.index(min(c.after)), "fewest rules, ties to the lowest k"
        k = len(out.kept)
        removed_any = removed_any or k < a.R0
        assert (rb[e, :nant, :k] == a.veval[:, out.kept]).all() and (rb[e, nant, :k] == a.rconc[out.kept]).all()
        assert (rant[e, :, :k] == a.rant[out.kept].T).all() and (uidx[e, :, :k] == a.uidx[:, out.kept]).all()
        assert (rb[e, :, k: a.R0] == 0).all() and (rant[e, :, k: a.R0] == 0).all() and (uidx[e, :, k: a.R0] == 0).all(), "vacated tail zeroed"
        assert (rb[e, :, a.R0:] == SENTINEL).all() and (rant[e, :, a.R0:] == SENTINEL).all() and (uidx[e, :, a.R0:] == 3).all()
    assert removed_any


@pytest.mark.parametrize("resident", [1, 0])
def test_orders_many_points_in_several_passes(resident, hip_option):
    import torch
    c = SYNTH_REDUCE
    b, ave, avals, pts, cases, diag = synth_reference()
    print("synth min_rel_gap", diag.min_rel_gap, "after", [x.after for x in cases], "chosen", [x.chosen for x in cases])
    check_margin(diag)
    prob = b.to_device(device(), compressed=True)
    agent = synth_agent(b, ave, avals, 0)
    points, count = tens(pts), tens(np.array(c["counts"], dtype=np.int32))
    hip_option("reduce_map_resident", resident)
    best0, _ = prob.policy_map(agent, points, point_count=count, actconc=False)
    res, kept, after = prob.reduce_batch_map_orders(agent, points, tens(orders_tensor(cases, prob.maxR)), point_count=count)
    best1, _ = prob.policy_map(agent, points, point_count=count, actconc=False)
    torch.cuda.synchronize()
    assert (best1.cpu().numpy() == best0.cpu().numpy()).all()
    rb, uidx, nant = prob.rb.cpu().numpy(), prob.uidx.cpu().numpy(), c["nant"]
    for e, x in enumerate(cases):
        k = len(x.out.kept)
        assert list(after[e]) == x.after
        assert (res[e].rules_before, res[e].rules_after, res[e].points, res[e].chosen, res[e].tries) == (c["R"], k, c["counts"][e], x.chosen, x.out.tries)
        assert list(kept[e]) == x.out.kept and 1 <= k < c["R"]
        assert (rb[e, :, :k] == b.rb[e][:, x.out.kept]).all() and (rb[e, :, k:] == 0).all()
        assert (uidx[e, :, :k] == b.uidx[e][:, x.out.kept]).all() and (uidx[e, :, k:] == 0).all()


def device_state(prob, rant_d):
    return [x.cpu().numpy().tobytes() for x in (prob.rb, prob.nrules, rant_d, prob.uidx)]


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("strategy", [1, 2])
@pytest.mark.parametrize("env", ENVS)
def test_one_order_from_rule_order_is_the_strategy(env, strategy, resident, hip_option):
    """K = 1 with frirl_hip_rule_order(keys = NULL) against frirl_hip_reduce_batch_map on another copy: bit-identical"""
    import torch
    pts = episode_points_on_device(env)
    agents, counts, active = mix(env)
    counts = counts(len(pts))
    E = len(agents)
    hip_option("reduce_map_resident", resident)
    agent = agent_for(env)
    state = []
    for which in ("strategy", "orders"):
        prob, rant_d, _ = upload(agents, with_uidx=True)
        points = tens(np.broadcast_to(pts, (E, len(pts), prob.nant - 1)))
        count_d, active_d = tens(np.array(counts, dtype=np.int32)), tens(np.array(active, dtype=np.uint8))
        if which == "strategy":
            res, kept = prob.reduce_batch_map(agent, points, point_count=count_d, active=active_d, strategy=strategy, rant=rant_d)
        else:
            order = prob.rule_order(None, descending=strategy == 2)
            res, kept, after = prob.reduce_batch_map_orders(agent, points, order.unsqueeze(1).contiguous(), point_count=count_d, active=active_d, rant=rant_d)
            assert [int(a[0]) for a in after] == [r.rules_after for r in res]
            assert [r.chosen for r in res] == [-1 if (not active[e] or counts[e] == 0 or agents[e].R0 == 1) else 0 for e in range(E)]
        torch.cuda.synchronize()
        state.append(([k.tolist() for k in kept], [(r.rules_before, r.rules_after, r.points, r.tries) for r in res], device_state(prob, rant_d)))
    assert state[0][0] == state[1][0] and state[0][1] == state[1][1], "kept, rules_after, tries"
    assert state[0][2] == state[1][2], "rule bases, nrules, rant, uidx: the same bits"
    assert any(r[1] < r[0] for r in state[0][1])


@pytest.mark.parametrize("what", ["duplicate", "index == R", "negative"])
def test_a_non_permutation_is_refused_before_anything_is_reduced(what):
    import torch
    env = "mountaincar"
    pts = episode_points_on_device(env)
    agents, counts, active = mix(env)
    counts = counts(len(pts))
    E = len(agents)
    prob, rant_d, _ = upload(agents, with_uidx=True)
    points = tens(np.broadcast_to(pts, (E, len(pts), prob.nant - 1)))
    count_d, active_d = tens(np.array(counts, dtype=np.int32)), tens(np.array(active, dtype=np.uint8))
    good = prob.rule_order(None)
    orders = torch.stack([good, good, good], dim=1).contiguous()
    R = agents[1].R0
    orders[1, 2, R // 2] = {"duplicate": int(orders[1, 2, 0]), "index == R": R, "negative": -1}[what]
    # the orders of agents that are left alone are not read: no point (2), inactive (3)
    orders[2, 1, :] = -5
    orders[3, 0, :] = 1 << 20
    before = device_state(prob, rant_d)
    with pytest.raises(frirl_amd.FrirlHipError, match=r"frirl_hip_reduce_batch_map_orders: agent 1, order k=2"):
        prob.reduce_batch_map_orders(agent_for(env), points, orders, point_count=count_d, active=active_d, rant=rant_d)
    torch.cuda.synchronize()
    assert device_state(prob, rant_d) == before, "every rule base as it was"
    # a bad rule count of an active agent is refused the same way
    prob.nrules[0] = prob.maxR + 1
    with pytest.raises(frirl_amd.FrirlHipError, match="agent 0: nrules outside"):
        prob.reduce_batch_map_orders(agent_for(env), points, torch.stack([good, good, good], dim=1).contiguous(), point_count=count_d, active=active_d,
                                     rant=rant_d)
    prob.nrules[0] = agents[0].R0
    torch.cuda.synchronize()
    assert device_state(prob, rant_d) == before
    # mended: the call goes through
    res, kept, after = prob.reduce_batch_map_orders(agent_for(env), points, torch.stack([good, good, good], dim=1).contiguous(), point_count=count_d,
                                                    active=active_d, rant=rant_d)
    assert res[0].chosen == 0 and res[0].rules_after < res[0].rules_before and res[2].chosen == -1 and res[3].chosen == -1


@pytest.mark.parametrize("env", ENVS + ["synth"])
def test_usage_order_reduce_end_to_end(env):
    """frirl_hip_rule_usage -> frirl_hip_rule_order(sum) -> frirl_hip_reduce_batch_map_orders on the device alone.  Every agent: the
    device's sums are the reference's within the Q tolerance, its order ranks the reference's sums within that tolerance, the map is
    preserved and the results are consistent.  An agent whose reference sums are >= 1e-6 apart without ties and whose reference run
    meets the margin condition (module docstring): the reference's order and kept list exactly."""
    import torch
    if env == "synth":
        b, ave, avals, pts, cases, _ = synth_reference()
        prob = b.to_device(device(), compressed=True)
        agent = synth_agent(b, ave, avals, 0)
        points, counts, active, rant_d = tens(pts), SYNTH_REDUCE["counts"], [1, 1], None
    else:
        p = episode_points_on_device(env)
        cases, _ = reference(env, tuple(map(tuple, p)))
        agents, counts, active = mix(env)
        counts = counts(len(p))
        prob, rant_d, _ = upload(agents, with_uidx=True)
        agent = agent_for(env)
        points = tens(np.broadcast_to(p, (len(agents), len(p), prob.nant - 1)))
    count_d, active_d = tens(np.array(counts, dtype=np.int32)), tens(np.array(active, dtype=np.uint8))
    best0, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    total, _, _ = prob.rule_usage(agent, points, point_count=count_d, active=active_d)
    order = prob.rule_order(total, active=active_d)
    res, kept, after = prob.reduce_batch_map_orders(agent, points, order.unsqueeze(1).contiguous(), point_count=count_d, active=active_d, rant=rant_d)
    best1, _ = prob.policy_map(agent, points, point_count=count_d, active=active_d, actconc=False)
    torch.cuda.synchronize()
    assert (best1.cpu().numpy() == best0.cpu().numpy()).all()
    total_h, order_h = total.cpu().numpy(), order.cpu().numpy()
    strict = 0
    for e, c in enumerate(cases):
        R = len(c.args[3])
        assert res[e].rules_before == R and res[e].rules_after == len(kept[e]) == int(after[e, 0])
        if c.untouched:
            assert res[e].chosen == -1 and list(kept[e]) == list(range(R)) and res[e].tries == 0
            continue
        want, want_order, out, diag = c.by_usage
        got = list(order_h[e, :R])
        assert (np.abs(total_h[e, :R] - want) <= 1e-9 * np.abs(want) + 1e-300).all()
        assert sorted(got) == list(range(R)) and (np.diff(want[got]) >= -1e-9 * want[got][1:]).all(), "the device ranks its sums; they are the reference's within 1e-9"
        assert res[e].chosen == 0 and list(kept[e]) == sorted(set(kept[e])) and set(kept[e]) <= set(range(R))
        ok = sums_are_apart(want) and diag.ties == 0 and diag.min_rel_gap >= 1e-6
        print(env, e, "sums apart", sums_are_apart(want), "min_rel_gap", diag.min_rel_gap, "reference keeps", len(out.kept), "device keeps", len(kept[e]))
        if ok:
            strict += 1
            assert got == want_order and list(kept[e]) == out.kept and res[e].tries == out.tries, e
    assert strict == STRICT[env]


def test_batch_object_order_sets():
    """order_set = 1 against frirl_hip_batch_reduce_all_map(strategy 1) on two identically built batches: bit-identical; order_set = 15 on
    a third: the best of four per agent, never worse than |Q| ascending alone, the greedy roll-outs that contributed reproduced"""
    import torch
    env, E, n, maxR, nant = "mountaincar", 4, 4, 512, 3
    L = frirl_amd.lib()
    probe = ob.Frirl(env, trig_mode=1)
    own = spread_starts(probe, E, 0.15)
    rows = np.stack([spread_starts(probe, n, 0.15, seed=60 + e) for e in range(E)])
    rows[:, 0] = own
    batches = [frirl_amd.demo_batch_object(env, E, maxR, start_states=own) for _ in range(3)]
    try:
        eps = C.c_int32(-1)
        for b in batches:
            frirl_amd.check(L.frirl_hip_batch_train(b, 40, C.byref(eps)), "frirl_hip_batch_train")
        before = [[rulebase_of(b, e, nant, maxR) for e in range(E)] for b in batches]
        for x in before[1:]:
            assert all(p[0] == q[0] and same_bits(p[1], q[1]) and same_bits(p[2], q[2]) for p, q in zip(before[0], x)), "identically built"
        res_s, tot_s = frirl_amd.batch_reduce_all_map(batches[0], 1, n, rows)
        res_1, after_1, tot_1 = frirl_amd.batch_reduce_all_map_orders(batches[1], 1, n, rows)
        res_f, after_f, tot_f = frirl_amd.batch_reduce_all_map_orders(batches[2], 15, n, rows)
        got = [[rulebase_of(b, e, nant, maxR) for e in range(E)] for b in batches]
        assert all(p[0] == q[0] and same_bits(p[1], q[1]) and same_bits(p[2], q[2]) for p, q in zip(got[0], got[1])), "order_set 1 = strategy 1"
        assert [(r.rules_before, r.rules_after, r.points, r.tries) for r in res_s] == [(r.rules_before, r.rules_after, r.points, r.tries) for r in res_1]
        assert after_1.shape == (E, 1) and [int(a) for a in after_1[:, 0]] == [r.rules_after for r in res_1]
        for f in ("agents_reduced", "agents_overflow", "agents_without_points", "rules_before", "rules_after", "points"):
            assert getattr(tot_s, f) == getattr(tot_1, f), f
        assert after_f.shape == (E, 4)
        print("after_per_order", after_f.tolist(), "chosen", [r.chosen for r in res_f])
        for e in range(E):
            r = res_f[e]
            assert r.rules_before == before[2][e][0] and r.points == res_1[e].points
            if r.chosen < 0:
                assert r.rules_after == r.rules_before and (after_f[e] == r.rules_before).all()
                continue
            assert r.rules_after == int(after_f[e].min()) == got[2][e][0] and r.chosen == int(np.argmin(after_f[e])) and r.rules_after <= res_1[e].rules_after
            assert int(after_f[e, 0]) == res_1[e].rules_after, "order 0 of the set is |Q| ascending"
        assert tot_f.agents_reduced == sum(r.rules_after < r.rules_before for r in res_f) > 0 and tot_f.agents_overflow == 0
        assert tot_f.rules_before == sum(r.rules_before for r in res_f) and tot_f.rules_after == sum(r.rules_after for r in res_f)
        assert tot_f.points == sum(r.points for r in res_f) == tot_1.points > 0
        # the map at every agent's points is preserved: the greedy roll-outs from the successful starts are reproduced on the reduced rule bases
        agent = agent_for(env)
        starts = tens(rows.reshape(E * n, nant - 1))
        runs = []
        for rbs in (before[2], got[2]):
            prob, _, _ = upload([Trained(env, own[e], rules=(rbs[e][1], rbs[e][2])) for e in range(E)], maxR=maxR)
            runs.append([x.cpu().numpy() for x in prob.rollout_batch(agent, n, start_states=starts)[:3]])
        torch.cuda.synchronize()
        sel = runs[0][2] == 1
        assert sel.any() and (runs[1][0][sel] == runs[0][0][sel]).all() and (runs[1][2][sel] == 1).all() and same_bits(runs[1][1][sel], runs[0][1][sel])
        assert L.frirl_hip_batch_train(batches[2], 3, C.byref(eps)) == 0, L.frirl_hip_last_error()
    finally:
        for b in batches:
            L.frirl_hip_batch_destroy(b)
