"""The caller-stepped reduction of EVERY agent's rule base against a set of start states on the GPU:
frirl_hip_batch_reducer_create_starts / _result_starts (csrc/policy_batch.hip; the step kernel's PolicyStartsArgs form in
csrc/policy_batch_kernel.h, the STEPPED close kernel in csrc/reduce_starts_kernels.h).

1. The demos, stepped (frirl_hip_env_step plays the caller's environment) against the in-kernel frirl_hip_reduce_batch_starts on the same
   inputs: kept, results, per-start results and the device state.
2. n = 1: a reducer made by _create_starts equals one made by _create exactly.
3. Shapes no demo has (PointEnv): the test drives the rounds, books every row itself and derives the expected removals from its books.
4. The round protocol on a reducer with start states.

Row layout (include/frirl_hip.h): round 0 row e * n + k, later row (e * nodes + node) * n + k; e = q // rows_per_agent, k = q % n.

Stepped against in-kernel the comparisons are exact except rewards (1e-9 relative, as tests/test_hip_policy_batch.py)."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import reduce_starts_ref as ref
from tests.test_hip_policy_batch import FIELDS, POINT_SHAPES, assert_same_reduction, demo_step_fn, point_batch, same
from tests.test_hip_reduce_batch import Trained, agent_for, case, upload
from tests.test_hip_reduce_starts import RAGGED_COUNT, acrobot_starts, mixed_starts, ragged_starts, run_starts, starts_around, tens

pytestmark = pytest.mark.gpu
DEV = "cuda"


def start_rows(S, Q, rows_per_agent, n):
    """the observations a caller resets its Q environments to: S [E, n, nant-1], row q = start q % n of agent q // rows_per_agent"""
    import torch
    q = torch.arange(Q, device=S.device)
    return S[q // rows_per_agent, q % n].contiguous()


def run_stepped_starts(env, agents, starts, strategy, depth, count=None, drop=False, with_uidx=False, active=None):
    import torch
    prob, rant_d, host = upload(agents, with_uidx)
    agent = agent_for(env)
    S = tens(np.asarray(starts, dtype=np.float64))
    act = None if active is None else tens(np.asarray(active, dtype=np.uint8))
    cnt = None if count is None else tens(np.asarray(count, dtype=np.int32))
    kept, res, per = frirl_amd.reduce_external_batch_starts(prob, agent, lambda Q, rpa, n: start_rows(S, Q, rpa, n), demo_step_fn(agent, env), strategy,
                                                            S.shape[1], 0.0, depth, rant=rant_d, active=act, start_count=cnt, drop_bad_starts=drop)
    torch.cuda.synchronize()
    return kept, res, per, prob, rant_d, host


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def assert_same_starts_reduction(got, want):
    """stepped (kept, res, per, prob, rant) against in-kernel: kept, FIELDS, rb / nrules / uidx / rant exactly, rewards within 1e-9 relative
    (assert_same_reduction); per start `used` and `steps_incremental` exactly, its two rewards within the same bound"""
    assert_same_reduction((got[0], got[1], got[3], got[4]), (want[0], want[1], want[3], want[4]))
    for e, (pa, pb) in enumerate(zip(got[2], want[2])):
        assert len(pa) == len(pb)
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert (a.used, a.steps_incremental) == (b.used, b.steps_incremental), (e, k)
            assert close(a.baseline_reward, b.baseline_reward) and close(a.reward, b.reward), (e, k)


def both(env, agents, starts, strategy, depth, **kw):
    got = run_stepped_starts(env, agents, starts, strategy, depth, **kw)
    want = run_starts(env, agents, starts, strategy, depth, **kw)
    assert_same_starts_reduction(got, want)
    return got


# ---- 1. the demos: stepped = in-kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,depth,with_uidx", [(1, 2, True), (2, 4, False)])
def test_mountaincar_ragged_starts(strategy, depth, with_uidx):
    """E = 3, n = 3, start_count = [3, 1, 2].  Depth 2: 9 rows per agent with 8 rule slices and 4 lanes per row (8 rows per workgroup):
    two workgroups per agent, holes (starts that take no part) inside the first.  Depth 4: 45 rows, six workgroups per agent."""
    kept, res, per, _, _, _ = both("mountaincar", case("mountaincar")[:3], ragged_starts(), strategy, depth, count=RAGGED_COUNT, with_uidx=with_uidx)
    assert [[p.used for p in pe] for pe in per] == [[1, 1, 1], [1, 0, 0], [1, 1, 0]]
    assert [[p.steps_incremental >= 0 for p in pe] for pe in per] == [[True] * 3, [True, False, False], [True, True, False]]
    assert all(r.rules_after < r.rules_before for r in res)


def test_mountaincar_with_an_inactive_agent():
    agents = case("mountaincar")[:3]
    kept, res, per, _, _, _ = both("mountaincar", agents, ragged_starts(), 1, 4, count=RAGGED_COUNT, with_uidx=True, active=[1, 0, 1])
    assert (res[1].rounds, res[1].rollouts, res[1].rules_after) == (0, 0, agents[1].R0) and (kept[1] == np.arange(agents[1].R0)).all()
    assert [(p.used, p.steps_incremental, p.baseline_reward, p.reward) for p in per[1]] == [(0, -1, 0.0, 0.0)] * 3
    assert res[0].rules_after < res[0].rules_before and res[2].rules_after < res[2].rules_before


@pytest.mark.parametrize("drop", [False, True])
def test_acrobot_bad_starts_block_or_are_dropped(drop):
    """n = 4: good, bad, good, bad.  drop_bad_starts = 0: the bad starts stay in and block every removal.  1: they are dropped on the device
    after the baseline, so rows of the two good starts, with different caps, share workgroups with the holes of the bad ones."""
    agents = case("acrobot")[:2]
    kept, res, per, _, _, _ = both("acrobot", agents, mixed_starts(), 1, 10, drop=drop)
    for e, a in enumerate(agents):
        assert [p.used for p in per[e]] == ([1, 0, 1, 0] if drop else [1, 1, 1, 1])
        assert (res[e].rules_after < a.R0) if drop else (res[e].rules_after == a.R0 and res[e].rounds == -(-a.R0 // 10))
    if drop:
        caps = {p.steps_incremental for pe in per for p in pe if p.used}
        assert len(caps) > 1, caps


def test_agent_with_only_bad_starts_finishes_after_the_baseline():
    """drop_bad_starts = 1 and four bad starts for agent 1: rounds == 0, and every row of it is done after begin in every later round"""
    import torch
    agents = case("acrobot")[:2]
    (g0, b0), (g1, b1) = acrobot_starts()
    starts = np.stack([np.stack([g0[0], b0[0], g0[1], b0[1]]), b1[:4]])
    want = run_starts("acrobot", agents, starts, 1, 10, drop=True)
    prob, rant_d, _ = upload(agents)
    agent = agent_for("acrobot")
    S = tens(starts)
    step_fn = demo_step_fn(agent, "acrobot")
    red = frirl_amd.BatchReducer(prob, agent, 1, 0.0, 10, rant_d, starts=4, drop_bad_starts=True)
    later_rounds = 0
    try:
        while red.next_round() > 0:
            states = start_rows(S, red.Q, red.rows_per_agent, 4)
            action, _ = red.begin(states)
            if red.rows_per_agent > 4:
                later_rounds += 1
                assert red.agents_live == 1 and bool((red.row_done()[red.rows_per_agent:] == 1).all())
            live = red.Q
            while live > 0:
                out = step_fn(states, action)
                action, _, live = red.observe(out[0], out[1], out[2])
                states = out[0]
            red.end_round()
        got = red.result() + (red.result_starts(), prob, rant_d)
    finally:
        red.close()
    torch.cuda.synchronize()
    assert_same_starts_reduction(got, want)
    r1 = got[1][1]
    assert later_rounds > 0 and (r1.rules_before, r1.rules_after, r1.rounds, r1.rollouts) == (agents[1].R0, agents[1].R0, 0, 4)
    assert [p.used for p in got[2][1]] == [0, 0, 0, 0] and all(p.steps_incremental > 0 for p in got[2][1])


def test_cartpole_one_rule_base_two_start_states():
    """21 actions: 8 lanes per row; the environment's own quantiser arrives as q_obs"""
    first, second = case("cartpole")
    starts = np.stack([first.start, second.start])[None]
    kept, res, per, _, _, _ = both("cartpole", [first], starts, 1, 0)
    assert per[0][0].steps_incremental != per[0][1].steps_incremental or per[0][0].baseline_reward != per[0][1].baseline_reward
    assert res[0].rules_after < res[0].rules_before


def test_tiny_rule_base_next_to_a_normal_one():
    """An agent with 4 rules (one round whose tree has 2^4 - 1 of the 2^6 - 1 nodes: the rows of the other 48 nodes are holes) beside a
    110-rule agent, two starts each"""
    normal = case("mountaincar")[0]
    fr = ob.Frirl("mountaincar", trig_mode=1)                         # untrained: the 2^3 corner rules
    tiny = Trained("mountaincar", normal.start, rules=(np.array(fr.five.rant[:4]), np.array(fr.five.rconc[:4])))
    starts = np.stack([starts_around("mountaincar", normal.start, 2, 0.4, 51)] * 2)
    kept, res, per, _, _, _ = both("mountaincar", [tiny, normal], starts, 1, 6)
    K = sum(p.used for p in per[0])
    assert res[0].rounds == (1 if K else 0) and res[0].rollouts == 2 + 15 * K
    assert res[1].rules_after < res[1].rules_before


# ---- 2. one start state: the reducer made without start states ----------------------------------------------------------------------
def assert_one_start_equals_plain(clone, agent, S, step_fn, depth):
    """clone() -> (Problem, rant) of the same inputs.  kept, every result field with the reward's bits, rb / nrules / uidx / rant; and the
    n = 1 view of the plain reducer's result_starts equals the per-start results of the other"""
    import torch
    outs = []
    for starts in (None, 1):
        prob, rant = clone()
        red = frirl_amd.BatchReducer(prob, agent, 1, 0.0, depth, rant, starts=starts)
        assert red.starts == 1
        kept, res, per = frirl_amd._reduce_rounds(red, lambda r: start_rows(S, r.Q, r.rows_per_agent, 1), step_fn,
                                                  result=lambda r: r.result() + (r.result_starts(),))
        torch.cuda.synchronize()
        outs.append((kept, res, per, prob, rant))
    (k0, r0, p0, prob0, rant0), (k1, r1, p1, prob1, rant1) = outs
    for e in range(len(k0)):
        assert len(k0[e]) == len(k1[e]) and (k0[e] == k1[e]).all(), e
        for f in FIELDS + ("reserved",):
            assert getattr(r0[e], f) == getattr(r1[e], f), (e, f)
        assert np.float64(r0[e].reward).view(np.int64) == np.float64(r1[e].reward).view(np.int64), e
        assert [(p.used, p.steps_incremental, p.baseline_reward, p.reward) for p in p0[e]] == [(p.used, p.steps_incremental, p.baseline_reward, p.reward) for p in p1[e]]
        assert p1[e][0].used == 1 and p1[e][0].steps_incremental == r1[e].steps_incremental and p1[e][0].reward == r1[e].reward
    assert same(prob0.rb, prob1.rb) and same(prob0.nrules, prob1.nrules) and same(prob0.uidx, prob1.uidx) and same(rant0, rant1)
    return r1


def test_one_start_equals_the_plain_reducer_mountaincar_depth_4():
    agents = case("mountaincar")[:3]
    agent = agent_for("mountaincar")
    S = tens(np.stack([a.start for a in agents])[:, None, :])
    res = assert_one_start_equals_plain(lambda: upload(agents, True)[:2], agent, S, demo_step_fn(agent, "mountaincar"), 4)
    assert all(r.rules_after < r.rules_before for r in res)


def test_one_start_equals_the_plain_reducer_point_shape(hip_option):
    hip_option("policy_slices", 1)
    pb = point_batch(4, 5)
    S = tens(np.stack(pb.starts)[:, None, :])
    res = assert_one_start_equals_plain(pb.clone, pb.agent, S, pb.step_fn, 10)
    assert all(1 <= r.rules_after < r.rules_before for r in res)


# ---- 3. shapes no demo has: the test keeps the books --------------------------------------------------------------------------------
# The two extra start states of every agent: point_starts' draw with these seeds.  Chosen on the CPU with rule bases the oracle learned
# from the agents' own start states (Mirror of tests/test_hip_external.py, as POINT_SEEDS): its sequential reduction against the three
# starts meets no arg-max near-tie, and per agent it removes / has a candidate that start 0 accepts and another start rejects --
# (2, 3): 2, 2, 1 removed / 1, 2, 2 such candidates; (4, 5): 41, 55, 14 / 9, 9, 34; (8, 3): 276, 309, 322 / 0, 15, 11.
# On an MI355X, with the rule bases learned there (point_batch): (2, 3) keeps 4, 3, 6 of 6, 6, 7 rules with 6 such nodes along the walks;
# (4, 5) keeps 15, 15, 36 of 56, 70, 50 with 52; (8, 3) keeps 5, 35, 31 of 281, 344, 353 with 26.
EXTRA_SEEDS = (22, 23)
POINT_DEPTH = 4


def point_start_sets(pb, nant, A):
    extra = [np.random.default_rng(1000 * seed + nant * 100 + A).uniform(-0.9, 0.9, nant - 1) for seed in EXTRA_SEEDS]
    return np.ascontiguousarray(np.stack([np.stack([s] + extra) for s in pb.starts]))


@pytest.mark.parametrize("nant,A", POINT_SHAPES)
def test_point_shapes_follow_the_books_the_test_keeps(nant, A):
    """n = 3 starts per agent, default lane shapes.  The test books every row's steps and reward from what its own environment returned
    (float64, in step order), requires every row to go `done` exactly at success or at its start's cap, and after every round derives
    the removals from its books with the model's walk and candidate order.  Nothing depends on which action won an arg-max."""
    import torch
    pb = point_batch(nant, A)
    d, E, n, depth, nodes = pb.d, pb.E, 3, POINT_DEPTH, (1 << POINT_DEPTH) - 1
    good, max_steps = d["reward_good_above"], d["max_steps"]
    prob, rant = pb.clone()
    rb0, rant0, uidx0 = prob.rb.cpu().numpy().copy(), rant.cpu().numpy().copy(), prob.uidx.cpu().numpy().copy()
    R0 = [int(r) for r in prob.nrules.cpu().numpy()]
    S = tens(point_start_sets(pb, nant, A))
    order = [ref.candidate_order(rb0[e, nant, : R0[e]], 1) for e in range(E)]
    alive, j = [list(range(R0[e])) for e in range(E)], [0] * E
    base = prev = caps = None
    blocked_by_another_start = 0
    wrong_done = torch.zeros((), dtype=torch.int64, device=DEV)
    red = frirl_amd.BatchReducer(prob, pb.agent, 1, 0.0, depth, rant, starts=n)
    try:
        rnd = 0
        while red.next_round() > 0:
            Q, rpa = red.Q, red.rows_per_agent
            assert rpa == (n if rnd == 0 else nodes * n) and Q == E * rpa
            q = torch.arange(Q, device=DEV)
            e_of, k_of, node_of = q // rpa, q % n, (q % rpa) // n
            if rnd == 0:
                exists = torch.ones(Q, dtype=torch.bool, device=DEV)
                cap = torch.full((Q,), max_steps, dtype=torch.int32, device=DEV)
            else:
                d_e = [max(min(depth, R0[e] - j[e]), 0) for e in range(E)]
                exists = node_of < torch.tensor([(1 << x) - 1 for x in d_e], device=DEV)[e_of]
                cap = torch.tensor(caps, dtype=torch.int32, device=DEV)[e_of, k_of]
            states = start_rows(S, Q, rpa, n)
            action, _ = red.begin(states)
            done = ~exists
            assert torch.equal(red.row_done() != 0, done), rnd
            steps = torch.zeros(Q, dtype=torch.int32, device=DEV)
            reward = torch.zeros(Q, dtype=torch.float64, device=DEV)
            live, calls = int(exists.sum()), 0
            while live > 0:
                was_live = ~done
                obs, r, ok = pb.step_fn(states, action)
                action, _, live = red.observe(obs.contiguous(), r.contiguous(), ok.to(torch.int32).contiguous())
                steps = steps + was_live.to(torch.int32)
                reward = torch.where(was_live, reward + r, reward)
                done = done | (was_live & (ok | (steps >= cap)))
                wrong_done += ((red.row_done() != 0) != done).sum()
                states = obs.contiguous()
                calls += 1
                assert calls <= max_steps, "rows are still live beyond max_steps"
            assert bool(done.all()) and int(wrong_done) == 0, rnd
            red.end_round()
            st_h, rw_h = steps.cpu().numpy(), reward.cpu().numpy()
            if rnd == 0:
                base = [[(int(st_h[e * n + k]), float(rw_h[e * n + k])) for k in range(n)] for e in range(E)]
                prev = [[b[1] for b in base[e]] for e in range(E)]
                caps = [[min(max_steps, b[0] + 1) for b in base[e]] for e in range(E)]
            else:
                for e in range(E):
                    de = min(depth, R0[e] - j[e])
                    if de <= 0:
                        continue
                    row = lambda node, k: (e * nodes + node) * n + k
                    st = [[int(st_h[row(node, k)]) for k in range(n)] for node in range((1 << de) - 1)]
                    rw = [[float(rw_h[row(node, k)]) for k in range(n)] for node in range((1 << de) - 1)]
                    inc = [b[0] for b in base[e]]
                    bits_, after = ref.walk(de, n, st, rw, inc, prev[e], good, 0.0)
                    # along the walk: nodes that start 0 accepts and another start rejects
                    b, p = 0, list(prev[e])
                    for kk in range(de):
                        node = (1 << kk) - 1 + b
                        ok_k = [ref.accept(st[node][k], rw[node][k], inc[k], p[k], good, 0.0) for k in range(n)]
                        if all(ok_k):
                            b |= 1 << kk
                            p = list(rw[node])
                        elif ok_k[0]:
                            blocked_by_another_start += 1
                    assert b == bits_ and p == after
                    gone = {order[e][j[e] + i] for i in range(de) if (bits_ >> i) & 1}
                    alive[e] = [x for x in alive[e] if x not in gone]
                    prev[e], j[e] = after, j[e] + de
            rnd += 1
        kept, res = red.result()
        per = red.result_starts()
    finally:
        red.close()
    torch.cuda.synchronize()
    print(f"point nant={nant} A={A}: rules {R0} -> {[len(a) for a in alive]}, {blocked_by_another_start} nodes accepted by start 0 and rejected by another")
    for e in range(E):
        R1 = len(alive[e])
        assert list(kept[e]) == alive[e], e
        assert (res[e].rules_before, res[e].rules_after, int(prob.nrules[e])) == (R0[e], R1, R1)
        assert (res[e].rounds, res[e].rollouts) == ref.counters(R0[e], depth, n, n), e
        assert (res[e].steps_incremental, res[e].reward) == (base[e][0][0], prev[e][0]), e
        assert [(p.used, p.steps_incremental, p.baseline_reward, p.reward) for p in per[e]] == [(1, base[e][k][0], base[e][k][1], prev[e][k]) for k in range(n)], e
        for got, orig in ((prob.rb[e].cpu().numpy(), rb0[e]), (rant[e].cpu().numpy(), rant0[e]), (prob.uidx[e].cpu().numpy(), uidx0[e])):
            assert (got[:, :R1] == orig[:, alive[e]]).all() and (got[:, R1: R0[e]] == 0).all() and (got[:, R0[e]:] == orig[:, R0[e]:]).all(), e
    assert any(len(alive[e]) < R0[e] for e in range(E)), "no agent removed a rule"
    assert blocked_by_another_start >= 1, "no node was accepted by start 0 and rejected by another start"


# ---- 4. protocol ------------------------------------------------------------------------------------------------------------------
def test_protocol_and_row_done_on_a_reducer_with_start_states():
    """acrobot, n = 4 (good, bad, good, bad), drop_bad_starts = 1, depth 10: calls out of order are refused, observe without rows_live
    does not synchronise, and after every begin row_done marks exactly the holes: the two starts that are not used, the nodes beyond
    2^d_e - 1 (the agents' last rounds) and every row of the agent that has finished."""
    import torch
    agents = case("acrobot")[:2]
    n, depth, nodes = 4, 10, 1023
    prob, rant_d, _ = upload(agents)
    agent = agent_for("acrobot")
    S = tens(mixed_starts())
    step_fn = demo_step_fn(agent, "acrobot")
    L = frirl_amd.lib()
    snapshot = (prob.rb.clone(), prob.nrules.clone(), rant_d.clone())

    def unchanged():
        torch.cuda.synchronize()
        return same(prob.rb, snapshot[0]) and same(prob.nrules, snapshot[1]) and same(rant_d, snapshot[2])

    def finish(states, action, live):
        while live > 0:
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2])
            states = out[0]

    red = frirl_amd.BatchReducer(prob, agent, 1, 0.0, depth, rant_d, starts=n, drop_bad_starts=True)
    try:
        assert red.starts == n
        obs0 = start_rows(S, 2 * n, n, n)
        io, _, _ = frirl_amd._agent_io(prob, obs0, E=2 * n)
        zeros = (torch.zeros(2 * n, dtype=torch.float64, device=DEV), torch.zeros(2 * n, dtype=torch.int32, device=DEV))
        io_obs, _, _ = frirl_amd._agent_io(prob, obs0, None, zeros[0], zeros[1], E=2 * n)
        res = frirl_amd.ReduceResult()
        per = (frirl_amd.ReduceStartResult * (2 * n))()
        assert L.frirl_hip_batch_reducer_begin(red.h, C.byref(io)) == -2              # begin before next_round
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # observe outside a round
        assert L.frirl_hip_batch_reducer_end_round(red.h) == -2
        assert L.frirl_hip_batch_reducer_result_starts(red.h, per) == 0 and [p.steps_incremental for p in per] == [-1] * (2 * n)   # before round 0
        assert red.next_round() == 2 * n and red.rows_per_agent == n and red.agents_live == 2
        q = C.c_int32()
        assert L.frirl_hip_batch_reducer_next_round(red.h, C.byref(q), None, None) == -2   # next_round inside a round
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # observe before begin
        action, _ = red.begin(obs0)
        assert L.frirl_hip_batch_reducer_begin(red.h, C.byref(io)) == -2              # begin twice
        assert bool((red.row_done() == 0).all())                                      # every start takes part in the baseline
        assert L.frirl_hip_batch_reducer_end_round(red.h) == -2 and b"have not ended" in L.frirl_hip_last_error()
        assert L.frirl_hip_batch_reducer_result(red.h, None, C.byref(res)) == -2
        assert L.frirl_hip_batch_reducer_result_starts(red.h, per) == -2 and b"round is open" in L.frirl_hip_last_error()
        assert unchanged()
        states = obs0
        for _ in range(3):                                                            # no count, no synchronisation
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2], count_live=False)
            assert live is None
            states = out[0]
        out = step_fn(states, action)
        action, _, live = red.observe(out[0], out[1], out[2])
        assert live == int((red.row_done() == 0).sum()) == 2 * n
        finish(out[0], action, live)
        assert unchanged()
        red.end_round()
        used = [[p.used for p in pe] for pe in red.result_starts()]
        assert used == [[1, 0, 1, 0]] * 2
        # the try-remove rounds
        R0, j = [a.R0 for a in agents], [0, 0]
        seen_short_tree = seen_finished_agent = False
        first = True
        while red.next_round() > 0:
            Q, rpa = red.Q, red.rows_per_agent
            assert rpa == nodes * n and Q == 2 * rpa
            d_e = [max(min(depth, R0[e] - j[e]), 0) for e in range(2)]
            assert red.agents_live == sum(x > 0 for x in d_e)
            seen_short_tree |= any(0 < x < depth for x in d_e)
            seen_finished_agent |= d_e[0] == 0 and d_e[1] > 0
            rows = torch.arange(Q, device=DEV)
            e_of, k_of, node_of = rows // rpa, rows % n, (rows % rpa) // n
            exists = (node_of < torch.tensor([(1 << x) - 1 for x in d_e], device=DEV)[e_of]) & (k_of % 2 == 0)
            states = start_rows(S, Q, rpa, n)
            action, _ = red.begin(states)
            assert torch.equal(red.row_done() != 0, ~exists), j
            live = int(exists.sum())
            if first:
                first = False
                out = step_fn(states, action)
                action, _, live = red.observe(out[0], out[1], out[2])
                states = out[0]
                assert 0 < live <= int(exists.sum())
                assert L.frirl_hip_batch_reducer_end_round(red.h) == -2 and unchanged()   # rows are live: nothing is compacted
                assert L.frirl_hip_batch_reducer_result_starts(red.h, per) == -2
            finish(states, action, live)
            red.end_round()
            j = [j[e] + d_e[e] for e in range(2)]
        assert seen_short_tree and seen_finished_agent and j == R0
        kept, results = red.result()
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # after the last round
        assert red.next_round() == 0 and red.agents_live == 0
        assert all(r.rules_after < r.rules_before and r.rounds == -(-a.R0 // depth) for r, a in zip(results, agents))
    finally:
        red.close()
