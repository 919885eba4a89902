"""EVERY agent's own rule base in the caller's environment on the GPU: frirl_hip_policy_batch_begin / _observe and the resumable
batched reduction frirl_hip_batch_reducer_* (csrc/policy_batch.hip, csrc/policy_batch_kernel.h).

1. Stepped batch roll-outs (frirl_hip_env_step plays the caller's environment) equal the in-kernel roll-outs of frirl_hip_rollout_shared
   run agent by agent: steps, reward, success and final states bit for bit -- with exclude masks, rows that do not exist, an agent
   list, and every rule-slice shape.
2. The stepped reduction of the demos equals frirl_hip_reduce_batch on cloned inputs (kept, results, rb / rant / uidx / nrules).
3. Shapes no demo has (PointEnv): exactly the single-base stepped reducer per agent, and the sequential loop of the oracle.
4. The round protocol.

Comparisons between the stepped and the in-kernel form are exact except the final reward (1e-9 relative, as tests/test_hip_reduce_batch.py):
the replays' decisions are integers and rewards come from the environment, but the in-kernel baseline replay may sum its rules in
another slice order than the stepped one, so a pick could only differ inside an arg-max tie; none was observed."""
import ctypes as C
import functools

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests.test_hip_external import Mirror, PointEnv, generic_quantize, point_desc
from tests.test_hip_policy import train_point_agent
from tests.test_hip_reduce_batch import Trained, agent_for, case, run_batch, spread_starts, starts_tensor, upload
from tests.test_policy_host import SequentialReduction

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("rules_before", "rules_after", "rounds", "rollouts", "steps_incremental")


def bits(x):
    import torch
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def same(a, b):
    import torch
    return a is None and b is None or torch.equal(bits(a), bits(b))


def demo_step_fn(agent, env):
    def step_fn(states, action):
        obs, reward, success, q = frirl_amd.env_step(agent, action, states)
        return (obs, reward, success, q) if env == "cartpole" else (obs, reward, success)
    return step_fn


# ---- 1. stepped batch roll-outs = in-kernel roll-outs, agent by agent ------------------------------------------------------------
E1, N1 = 3, 5
SENT = -7


@functools.lru_cache(maxsize=None)
def rollout_case():
    """Three mountaincar rule bases, five start states each; per agent a slot table of its 8 largest and 8 smallest |Q| and five
    masks; the in-kernel reference (frirl_hip_rollout_shared on that agent's slab) without and with the masks.  Computed once."""
    import torch
    agents = case("mountaincar")[:E1]
    agent = agent_for("mountaincar")
    prob, _, _ = upload(agents)
    s = np.concatenate([spread_starts(a.fr, N1, 0.15, seed=30 + e) for e, a in enumerate(agents)])
    slot = np.full((E1, prob.maxR), 255, dtype=np.uint8)
    for e, a in enumerate(agents):
        order = np.argsort(np.abs(a.rconc), kind="stable")
        for sl, r in enumerate([int(r) for r in order[-8:][::-1]] + [int(r) for r in order[:8]]):
            slot[e, r] = sl
    masks = np.tile(np.array([0, 1, 0xff, 0xff00, 0xa5a5], dtype=np.uint32).view(np.int32), E1)
    s_d, slot_d, masks_d = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (s, slot, masks))
    ref = {}
    for masked in (False, True):
        out = []
        for e, a in enumerate(agents):
            p1, _, _ = upload([a], maxR=prob.maxR)
            sl = slice(e * N1, (e + 1) * N1)
            kw = dict(exclude_mask=masks_d[sl].contiguous(), rule_slot=slot_d[e].contiguous()) if masked else {}
            out.append(p1.rollout_shared(agent, N1, start_states=s_d[sl].contiguous(), **kw))
        ref[masked] = [torch.cat([o[i] for o in out]) for i in range(4)]          # steps, reward, success, final states
    torch.cuda.synchronize()
    assert not same(ref[False][0], ref[True][0]) or not same(ref[False][1], ref[True][1]), "the masks are not exercised"
    return prob, agent, s_d, slot_d, masks_d, ref


def drive_batch(prob, agent, rows, s, record=False, count_live=True):
    """Every existing row of `rows` to the end of its episode; returns (final states, action-index trace).  Rows the library never
    writes keep SENT in the action buffers."""
    import torch
    Q = rows.Q
    out = (torch.full((Q,), float(SENT), dtype=torch.float64, device=DEV), torch.full((Q,), SENT, dtype=torch.int32, device=DEV))
    if rows.rows_live is not None:
        rows.rows_live.zero_()
    action, aidx = prob.policy_batch_begin(agent, rows, s, out=out)
    if rows.rows_live is not None:
        assert int(rows.rows_live[0]) == int((rows.done == 0).sum())
    trace = [aidx.clone()] if record else None
    states = s.clone()
    for t in range(agent.desc.max_steps):
        live = rows.done == 0
        obs, reward, success, q = frirl_amd.env_step(agent, torch.where(live, action, torch.zeros_like(action)), states)
        if rows.rows_live is not None:
            rows.rows_live.zero_()
        prob.policy_batch_observe(agent, rows, obs, reward, success, out=out)
        states = torch.where(live[:, None], obs, states)
        if record:
            trace.append(torch.where(live, aidx, torch.full_like(aidx, -1)))
        if t % 25 == 24:
            left = int((rows.done == 0).sum())
            if rows.rows_live is not None:
                assert int(rows.rows_live[0]) == left, t
            if left == 0:
                break
    torch.cuda.synchronize()
    assert bool((rows.done != 0).all())
    return states, trace, out


def assert_rows_equal(rows, states, ref, sel):
    steps, reward, success, final = ref
    assert same(rows.ep_steps[sel], steps[sel]) and same(rows.success[sel], success[sel])
    assert same(rows.ep_reward[sel], reward[sel]) and same(states[sel], final[sel])


@pytest.mark.parametrize("masked", [False, True])
def test_stepped_batch_rollouts_equal_in_kernel_rollouts(masked, hip_option):
    import torch
    prob, agent, s, slot, masks, ref = rollout_case()
    kw = dict(exclude_mask=masks, rule_slot=slot) if masked else {}
    everything = torch.ones(E1 * N1, dtype=torch.bool, device=DEV)
    traces = {}
    for H in (0, 1, 4, 8):                                            # 0 = the shipped selection; the lanes per row follow from A
        hip_option("policy_slices", H)
        rows = frirl_amd.PolicyBatchRows(E1, N1, DEV, rows_live=torch.zeros(1, dtype=torch.int32, device=DEV), **kw)
        states, traces[H], _ = drive_batch(prob, agent, rows, s, record=True)
        assert_rows_equal(rows, states, ref[masked], everything)
    for H, tr in traces.items():
        assert len(tr) == len(traces[1]) and all(torch.equal(a, b) for a, b in zip(tr, traces[1])), f"actions differ with {H} rule slices"


@pytest.mark.parametrize("masked", [False, True])
def test_rows_that_do_not_exist_and_agents_that_are_not_named_are_never_touched(masked):
    import torch
    prob, agent, s, slot, masks, ref = rollout_case()
    kw = dict(exclude_mask=masks, rule_slot=slot) if masked else {}
    node = torch.arange(E1 * N1, device=DEV) % N1
    owner = torch.arange(E1 * N1, device=DEV) // N1
    counts = torch.tensor([5, 2, 0], dtype=torch.int32, device=DEV)
    cases = [(dict(row_count=counts), node < counts[owner].long()),
             (dict(agents=torch.tensor([2, 0], dtype=torch.int32, device=DEV)), owner != 1)]
    for extra, exists in cases:
        rows = frirl_amd.PolicyBatchRows(E1, N1, DEV, rows_live=torch.zeros(1, dtype=torch.int32, device=DEV), **extra, **kw)
        rows.done[~exists] = 1
        rows.ep_steps[~exists] = SENT
        rows.success[~exists] = SENT
        rows.ep_reward[~exists] = float(SENT)
        states, _, (action, aidx) = drive_batch(prob, agent, rows, s)
        assert_rows_equal(rows, states, ref[masked], exists)
        gone = ~exists
        assert bool((rows.done[gone] == 1).all()) and bool((rows.ep_steps[gone] == SENT).all()) and bool((rows.success[gone] == SENT).all())
        assert bool((rows.ep_reward[gone] == SENT).all()) and bool((action[gone] == SENT).all()) and bool((aidx[gone] == SENT).all())
        assert bool((aidx[exists] >= 0).all())


def test_step_cap_per_agent_ends_the_episodes():
    import torch
    prob, agent, s, slot, masks, ref = rollout_case()
    caps = torch.tensor([3, 1000, 7], dtype=torch.int32, device=DEV)
    rows = frirl_amd.PolicyBatchRows(E1, N1, DEV, step_cap=caps)
    drive_batch(prob, agent, rows, s)
    want = torch.minimum(ref[False][0], caps.repeat_interleave(N1))
    assert torch.equal(rows.ep_steps, want)


# ---- 2. the demos' reductions: stepped = in-kernel --------------------------------------------------------------------------------
def run_stepped(env, agents, strategy, depth, with_uidx=False, active=None):
    import torch
    prob, rant_d, host = upload(agents, with_uidx)
    agent = agent_for(env)
    starts = starts_tensor(agents)
    act = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to(DEV)
    kept, res = frirl_amd.reduce_external_batch(prob, agent, lambda Q, n: starts.repeat_interleave(n, 0), demo_step_fn(agent, env), strategy, 0.0,
                                                depth, rant=rant_d, active=act)
    torch.cuda.synchronize()
    return kept, res, prob, rant_d


def assert_same_reduction(got, want, exact_reward=False):
    kept_a, res_a, prob_a, rant_a = got[:4]
    kept_b, res_b, prob_b, rant_b = want[:4]
    assert len(kept_a) == len(kept_b)
    for e, (ka, kb) in enumerate(zip(kept_a, kept_b)):
        assert len(ka) == len(kb) and (ka == kb).all(), e
        for f in FIELDS:
            assert getattr(res_a[e], f) == getattr(res_b[e], f), (e, f, getattr(res_a[e], f), getattr(res_b[e], f))
        tol = 0.0 if exact_reward else 1e-9 * max(1.0, abs(res_b[e].reward))
        assert abs(res_a[e].reward - res_b[e].reward) <= tol, (e, res_a[e].reward, res_b[e].reward)
    assert same(prob_a.rb, prob_b.rb) and same(prob_a.nrules, prob_b.nrules) and same(prob_a.uidx, prob_b.uidx) and same(rant_a, rant_b)


@pytest.mark.parametrize("strategy,with_uidx,active", [(1, True, [1, 0, 1]), (2, False, None)])
def test_mountaincar_depth_4_two_workgroups_per_agent(strategy, with_uidx, active):
    """15 nodes with 8 rule slices and 4 lanes per row: two workgroups per agent, the second with a row that does not exist."""
    agents = case("mountaincar")[:3]
    got = run_stepped("mountaincar", agents, strategy, 4, with_uidx, active)
    want = run_batch("mountaincar", agents, strategy, 4, with_uidx, active)
    assert_same_reduction(got, want)
    assert sum(r.rules_after < r.rules_before for r in got[1]) == (2 if active else 3)
    if active:
        assert got[1][1].rounds == 0 and got[1][1].rollouts == 0 and got[1][1].rules_after == agents[1].R0


@pytest.mark.parametrize("strategy", [1, 2])
def test_mountaincar_depth_7_one_rule_slice(strategy, hip_option):
    """127 nodes per agent, one lane group per row without rule slices."""
    hip_option("policy_slices", 1)
    agents = case("mountaincar")[:3]
    assert_same_reduction(run_stepped("mountaincar", agents, strategy, 7), run_batch("mountaincar", agents, strategy, 7))


def test_one_agent_equals_the_single_base_stepped_reducer():
    import torch
    a = case("mountaincar")[1]
    agent = agent_for("mountaincar")
    start = torch.from_numpy(a.start).to(DEV)
    p1, rant1, _ = upload([a], with_uidx=True)
    k1, r1 = frirl_amd.reduce_external(p1, agent, lambda Q: start.expand(Q, len(a.start)).contiguous(), demo_step_fn(agent, "mountaincar"), 1, 0.0, 10,
                                       rant=rant1[0])
    torch.cuda.synchronize()
    got = run_stepped("mountaincar", [a], 1, 10, with_uidx=True)
    assert_same_reduction(got, ([k1], [r1], p1, rant1), exact_reward=True)
    assert 0 < r1.rules_after < r1.rules_before


def test_acrobot_agents_finish_in_different_rounds():
    agents = case("acrobot")[:2]
    got = run_stepped("acrobot", agents, 1, 0)
    assert_same_reduction(got, run_batch("acrobot", agents, 1, 0))
    assert got[1][0].rounds != got[1][1].rounds and all(r.rules_after < r.rules_before for r in got[1])


def test_cartpole_eight_lanes_per_row_and_the_callers_quantiser():
    """21 actions: 8 lanes per row; the environment's own quantiser arrives as q_obs.  One rule base from two start states."""
    agents = case("cartpole")
    got = run_stepped("cartpole", agents, 1, 0)
    assert_same_reduction(got, run_batch("cartpole", agents, 1, 0))
    assert got[1][0].steps_incremental != got[1][1].steps_incremental or got[1][0].reward != got[1][1].reward


def test_tiny_rule_base_next_to_a_normal_one():
    """An agent with 4 rules (a single round whose tree has 2^4 - 1 of the 2^6 - 1 nodes) beside a 110-rule agent."""
    normal = case("mountaincar")[0]
    fr = ob.Frirl("mountaincar", trig_mode=1)                         # untrained: the 2^3 corner rules
    tiny = Trained("mountaincar", normal.start, rules=(np.array(fr.five.rant[:4]), np.array(fr.five.rconc[:4])))
    got = run_stepped("mountaincar", [tiny, normal], 1, 6)
    assert_same_reduction(got, run_batch("mountaincar", [tiny, normal], 1, 6))
    assert got[1][0].rounds == 1 and got[1][0].rollouts == 1 + 15


# ---- 3. shapes no demo has ---------------------------------------------------------------------------------------------------------
POINT_SHAPES = [(2, 3), (4, 5), (8, 3)]
# Start-state seeds.  Chosen on the CPU with rule bases the oracle learned from the same start states (Mirror of tests/test_hip_external.py):
# its sequential reduction meets no arg-max near-tie and keeps 1 <= rules < R0 for every one of them -- (2, 3): 3 of 6, 3 of 6, 5 of 7;
# (4, 5): 15 of 56, 10 of 70, 9 of 50; (8, 3): 5 of 281, 28 of 344, 24 of 353; (3, 3) at Shepard power 2: 6 of 10, 12 of 20, 5 of 17.
# Many seeds of the one-dimensional shape (2, 3) tie or lose every rule; they were passed over.
POINT_SEEDS = {(2, 3): (1, 6, 11), (4, 5): (1, 2, 3), (8, 3): (1, 2, 3), (3, 3): (1, 2, 4)}


def point_starts(nant, A):
    return [np.ascontiguousarray(np.random.default_rng(1000 * seed + nant * 100 + A).uniform(-0.9, 0.9, nant - 1)) for seed in POINT_SEEDS[(nant, A)]]


class PointBatch:
    """E rule bases of PointEnv in one batch [E][nant+1][maxR], with their raw antecedents and index mirror; clone() for every run."""

    def __init__(self, d, env, starts, u, ve, rb, nrules, uidx, rant, p=0):
        self.d, self.env, self.starts, self.tensors, self.p = d, env, starts, (u, ve, rb, nrules, uidx, rant), p
        self.nant, self.E = d["nant"], len(starts)
        self.agent = frirl_amd.demo_agent(d, DEV, p=p)

    def clone(self, e=None):
        u, ve, rb, nrules, uidx, rant = self.tensors
        sl = slice(None) if e is None else slice(e, e + 1)
        prob = frirl_amd.Problem(u, ve, rb[sl].clone(), nrules[sl].clone(), None if uidx is None else uidx[sl].clone())
        return prob, rant[sl].clone()

    def step_fn(self, states, action):
        return self.env.step(__import__("torch"), states, action)

    def start_rows(self, Q, n):
        import torch
        return torch.from_numpy(np.repeat(np.stack(self.starts), n, axis=0)).to(DEV)


@functools.lru_cache(maxsize=None)
def point_batch(nant, A):
    import torch
    d, env, starts = point_desc(nant, A), PointEnv(nant - 1), point_starts(nant, A)
    parts = [train_point_agent(d, nant, s) for s in starts]
    prob0 = parts[0][0]
    cat = lambda xs: torch.cat(xs).contiguous()
    return PointBatch(d, env, starts, prob0.u, prob0.ve, cat([p.rb for p, _, _ in parts]), cat([p.nrules for p, _, _ in parts]),
                      cat([p.uidx for p, _, _ in parts]), cat([ev.rant for _, _, ev in parts]))


def single_reductions(pb, strategy, depth):
    import torch
    out = []
    for e in range(pb.E):
        prob, rant = pb.clone(e)
        start = torch.from_numpy(pb.starts[e]).to(DEV)
        kept, res = frirl_amd.reduce_external(prob, pb.agent, lambda Q: start.expand(Q, pb.nant - 1).contiguous(), pb.step_fn, strategy, 0.0, depth,
                                              rant=rant[0])
        out.append((kept, res, prob, rant))
    torch.cuda.synchronize()
    return out


def assert_batch_equals_singles(pb, strategy, depth):
    import torch
    prob, rant = pb.clone()
    kept, res = frirl_amd.reduce_external_batch(prob, pb.agent, pb.start_rows, pb.step_fn, strategy, 0.0, depth, rant=rant)
    torch.cuda.synchronize()
    for e, (k1, r1, p1, rant1) in enumerate(single_reductions(pb, strategy, depth)):
        assert len(kept[e]) == len(k1) and (kept[e] == k1).all(), e
        for f in FIELDS + ("reward",):
            assert getattr(res[e], f) == getattr(r1, f), (e, f)
        assert same(prob.rb[e], p1.rb[0]) and same(prob.nrules[e], p1.nrules[0]) and same(rant[e], rant1[0])
        assert prob.uidx is None or same(prob.uidx[e], p1.uidx[0])
    return kept, res


@pytest.mark.parametrize("nant,A", POINT_SHAPES)
def test_point_shapes_equal_the_single_base_reducer_exactly(nant, A, hip_option):
    """policy_slices = 1 on both sides: every conclusion sums its rules in rule order whatever the lanes per row, so the stepped batch
    and the stepped single-base reducer see the same bits."""
    hip_option("policy_slices", 1)
    assert_batch_equals_singles(point_batch(nant, A), 1, 10)


@pytest.mark.parametrize("nant,A", POINT_SHAPES)
def test_point_shapes_follow_the_sequential_loop(nant, A):
    """Default shapes: every agent whose sequential reduction (the oracle's pieces, tests/test_policy_host.py) meets no arg-max near-tie
    must keep the same rules; at most one agent of the shape may be left out for near-ties."""
    import torch
    pb = point_batch(nant, A)
    d, env = pb.d, pb.env
    prob, rant = pb.clone()
    rb0, rant0, R0s = prob.rb.cpu().numpy().copy(), rant.cpu().numpy().copy(), prob.nrules.cpu().numpy().copy()
    kept, res = frirl_amd.reduce_external_batch(prob, pb.agent, pb.start_rows, pb.step_fn, 1, 0.0, 0, rant=rant)
    torch.cuda.synchronize()

    def env_fn(states, action):
        x, r, ok = env.step(np, states[None], np.array([action]))
        return x[0], float(r[0]), int(ok[0]), generic_quantize(d, x[0])

    left_out = 0
    for e in range(pb.E):
        R0 = int(R0s[e])
        assert res[e].rules_before == R0 and 1 <= res[e].rules_after < R0, (e, res[e].rules_after, R0)
        seq = SequentialReduction(d["u"], d["ve"], rant0[e, :, :R0].T.copy(), rb0[e, nant, :R0].copy(), d["action_ve"], d["grids"][nant - 1],
                                  pb.starts[e], env_fn, d["max_steps"], d["reward_good_above"])
        kept_seq = seq.run(1)
        print(f"point nant={nant} A={A} agent {e}: {R0} -> {res[e].rules_after} rules, sequential {len(kept_seq)}, near ties {seq.near_ties} of {seq.picks}")
        if seq.near_ties:
            left_out += 1
            continue
        assert list(kept[e]) == kept_seq, e
        assert res[e].steps_incremental == seq.steps_incremental
        R1 = res[e].rules_after
        got = prob.rb[e].cpu().numpy()
        assert (got[:, :R1] == rb0[e][:, kept[e]]).all() and (got[:, R1:R0] == 0).all() and (got[:, R0:] == rb0[e][:, R0:]).all()
    assert left_out <= 1, left_out


def test_point_shape_at_shepard_power_2():
    """agent.p = 2 runs the run-time-power variants (no rule slices on either side): three rule bases the oracle learned at p = 2."""
    import torch
    nant, A, p = 3, 3, 2
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    starts = point_starts(nant, A)
    fives = []
    for s in starts:
        m = Mirror(d, s, 1024, p=p)
        for _ in range(30):
            m.episode(env, None)
            if m.converged:
                break
        fives.append(m.five)
    maxR = max(f.R for f in fives) + 8
    maxR += maxR & 1
    rb = torch.from_numpy(np.stack([f.device_layout(maxR) for f in fives])).to(DEV)
    nrules = torch.tensor([f.R for f in fives], dtype=torch.int32, device=DEV)
    rant = torch.zeros((3, nant, maxR), dtype=torch.float64, device=DEV)
    for e, f in enumerate(fives):
        rant[e, :, : f.R] = torch.from_numpy(np.ascontiguousarray(np.array(f.rant[: f.R]).T)).to(DEV)
    pb = PointBatch(d, env, starts, torch.from_numpy(d["u"]).to(DEV), torch.from_numpy(d["ve"]).to(DEV), rb, nrules, None, rant, p=p)
    kept, res = assert_batch_equals_singles(pb, 1, 10)
    assert all(1 <= r.rules_after < r.rules_before for r in res)


# ---- 4. protocol ------------------------------------------------------------------------------------------------------------------
def test_batch_reducer_calls_out_of_order_are_refused_and_row_done_marks_the_idle_rows():
    import torch
    env = "mountaincar"
    normal = case(env)[0]
    fr = ob.Frirl(env, trig_mode=1)
    tiny = Trained(env, normal.start, rules=(np.array(fr.five.rant[:4]), np.array(fr.five.rconc[:4])))
    agents = [normal, tiny, case(env)[1]]                              # agent 1: 4 rules, one round of 15 nodes; agent 2: inactive
    depth, n = 5, 31
    prob, rant_d, _ = upload(agents)
    agent = agent_for(env)
    starts = starts_tensor(agents)
    L = frirl_amd.lib()
    snapshot = (prob.rb.clone(), prob.nrules.clone(), rant_d.clone())

    def unchanged():
        torch.cuda.synchronize()
        return same(prob.rb, snapshot[0]) and same(prob.nrules, snapshot[1]) and same(rant_d, snapshot[2])

    active = torch.tensor([1, 1, 0], dtype=torch.uint8, device=DEV)
    red = frirl_amd.BatchReducer(prob, agent, 1, 0.0, depth, rant_d, active)
    step_fn = demo_step_fn(agent, env)
    try:
        obs0 = starts.contiguous()
        io, _, _ = frirl_amd._agent_io(prob, obs0, E=3)
        io_obs, _, _ = frirl_amd._agent_io(prob, obs0, None, torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV), E=3)
        res = frirl_amd.ReduceResult()
        assert L.frirl_hip_batch_reducer_begin(red.h, C.byref(io)) == -2              # begin before next_round
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # observe outside a round
        assert L.frirl_hip_batch_reducer_end_round(red.h) == -2
        assert red.next_round() == 3 and red.rows_per_agent == 1 and red.agents_live == 2
        q = C.c_int32()
        assert L.frirl_hip_batch_reducer_next_round(red.h, C.byref(q), None, None) == -2   # next_round inside a round
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # observe before begin
        action, _ = red.begin(obs0)
        assert L.frirl_hip_batch_reducer_begin(red.h, C.byref(io)) == -2              # begin twice
        assert torch.equal(red.row_done().cpu(), torch.tensor([0, 0, 1], dtype=torch.int32))      # the inactive agent's row
        assert L.frirl_hip_batch_reducer_end_round(red.h) == -2 and b"have not ended" in L.frirl_hip_last_error()
        assert L.frirl_hip_batch_reducer_result(red.h, None, C.byref(res)) == -2
        assert unchanged()
        # observe without a count does not synchronise; a later counted call reports the rows that are live
        states = obs0
        for _ in range(3):
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2], count_live=False)
            assert live is None
            states = out[0]
        out = step_fn(states, action)
        action, _, live = red.observe(out[0], out[1], out[2])
        states = out[0]
        assert live == int((red.row_done() == 0).sum()) == 2
        while live > 0:
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2])
            states = out[0]
        assert unchanged()
        red.end_round()
        # first try-remove round: agent 0 has 2^5 - 1 nodes, agent 1 (4 rules) 2^4 - 1, agent 2 none
        assert red.next_round() == 3 * n and red.rows_per_agent == n and red.agents_live == 2
        states = starts.repeat_interleave(n, 0)
        action, _ = red.begin(states)
        want = torch.ones(3 * n, dtype=torch.int32)
        want[:n] = 0
        want[n: n + 15] = 0
        assert torch.equal(red.row_done().cpu(), want)
        out = step_fn(states, action)
        action, _, live = red.observe(out[0], out[1], out[2])
        assert 0 < live <= n + 15
        assert L.frirl_hip_batch_reducer_end_round(red.h) == -2 and unchanged()       # rows are live: nothing is compacted
        while live > 0:
            states = out[0]
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2])
        red.end_round()
        # second try-remove round: agent 1 has finished (its 4 candidates were one round)
        assert red.next_round() == 3 * n and red.agents_live == 1
        states = starts.repeat_interleave(n, 0)
        action, _ = red.begin(states)
        want[n:] = 1
        assert torch.equal(red.row_done().cpu(), want)
        live = n
        while live > 0:
            out = step_fn(states, action)
            action, _, live = red.observe(out[0], out[1], out[2])
            states = out[0]
        red.end_round()
        while red.next_round() > 0:
            states = starts.repeat_interleave(red.rows_per_agent, 0)
            action, _ = red.begin(states)
            live = red.Q
            while live > 0:
                out = step_fn(states, action)
                action, _, live = red.observe(out[0], out[1], out[2])
                states = out[0]
            red.end_round()
        kept, results = red.result()
        final = (prob.rb.clone(), prob.nrules.clone())
        assert L.frirl_hip_batch_reducer_observe(red.h, C.byref(io_obs), None) == -2  # after the last round
        assert L.frirl_hip_batch_reducer_begin(red.h, C.byref(io)) == -2
        assert red.next_round() == 0 and red.agents_live == 0
        torch.cuda.synchronize()
        assert same(prob.rb, final[0]) and same(prob.nrules, final[1])
    finally:
        red.close()
    want_kept, want_res = run_batch(env, agents, 1, depth, active=[1, 1, 0])[:2]
    for e in range(3):
        assert (kept[e] == want_kept[e]).all() and results[e].rules_after == want_res[e].rules_after and results[e].rounds == want_res[e].rounds
    assert results[2].rounds == 0 and results[0].rules_after < results[0].rules_before
