"""Batched rule-base reduction (frirl_hip_reduce_batch, csrc/reduce_batch.hip): every rule base of a batch reduced in one run of
try-remove rounds, each agent replaying from its own start state -- against the oracle's sequential reduction (orc_reduce_run =
frirl_sequential_run.c:170-350) agent by agent, against the single-base path (frirl_hip_reduce_shared) and for the device state it
leaves behind.  The rule bases are trained by the oracle on the CPU, once per environment.

Arg-max ties: the comparisons below are exact (same surviving rules, bit-equal, in the same order), so no replay may differ from the
oracle's at all; observed on an MI355X: 0 picks resolved differently in any case of this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob

pytestmark = pytest.mark.gpu

SENTINEL = 7.25          # written beyond every agent's rules before a call: those columns must come back untouched


def spread_starts(fr, E, spread, seed=11):
    """values_def +- spread * span (clipped), row 0 = values_def -- the draw order of tests/test_hip_shared.py: start_states"""
    rng = np.random.default_rng(seed)
    s = np.zeros((E, fr.nstates))
    for k in range(fr.nstates):
        d = fr.dim(k)
        vals = d["values"]
        s[:, k] = np.clip(d["values_def"] + rng.uniform(-spread, spread, E) * (vals[-1] - vals[0]), vals[0], vals[-1])
        s[0, k] = d["values_def"]
    return s


class Trained:
    """One agent's rule base as the oracle learned it, and the oracle itself (its rule base is restored before every reduction)."""

    def __init__(self, env, start, fr=None, rules=None):
        self.env, self.start = env, np.array(start)
        self.fr = fr or ob.Frirl(env, trig_mode=1)
        self.fr.set_start_state(self.start)
        if fr is None and rules is None:
            self.fr.run()                                              # agents that hit the episode limit are reduced as they are
        f = self.fr.five
        if rules is not None:
            self.restore(*rules)
        R = self.R0 = f.R
        self.rant, self.rconc = np.array(f.rant[:R]), np.array(f.rconc[:R])
        self.veval, self.uidx = np.array(f.veval[:, :R]), np.array(f.uidx[:, :R]).astype(np.int16)
        self._reduced = {}

    def restore(self, rant, rconc):
        f = self.fr.five
        while f.R:
            f.remove_rule(f.R - 1)
        for r in range(len(rconc)):
            f.add_rule(rant[r], rconc[r])
        assert f.R == len(rconc) and (np.array(f.rconc[: f.R]) == rconc).all() and (np.array(f.rant[: f.R]) == rant).all()

    def baseline(self):
        self.restore(self.rant, self.rconc)
        self.fr.set_start_state(self.start)
        self.fr.episode_eval()
        return self.fr.ep_steps, self.fr.ep_reward

    def reduced(self, strategy):
        """(rant, rconc) after the oracle's sequential reduction from this agent's start state; computed once"""
        if strategy not in self._reduced:
            self.restore(self.rant, self.rconc)
            self.fr.set_start_state(self.start)
            self.fr.reduce(strategy, 0.0)
            R = self.fr.five.R
            self._reduced[strategy] = (np.array(self.fr.five.rant[:R]), np.array(self.fr.five.rconc[:R]))
        return self._reduced[strategy]


@functools.lru_cache(maxsize=None)
def case(env):
    """The cases: mountaincar E = 6 (spread 0.15), acrobot E = 4 (0.05), each agent trained from its own start state; cartpole
    E = 2 (0.02): the default agent's rule base twice, with two start states whose baseline episodes differ."""
    probe = ob.Frirl(env, trig_mode=1)
    if env == "cartpole":
        first = Trained(env, spread_starts(probe, 2, 0.02)[0])
        base0 = first.baseline()
        for seed in range(11, 40):
            s = spread_starts(probe, 2, 0.02, seed)
            second = Trained(env, s[1], rules=(first.rant, first.rconc))
            if second.baseline() != base0:
                return [first, second]
        raise AssertionError("no start state found whose baseline episode differs from the default one")
    E, spread = {"mountaincar": (6, 0.15), "acrobot": (4, 0.05)}[env]
    s = spread_starts(probe, E, spread)
    agents = [Trained(env, s[e]) for e in range(E)]
    want = {"mountaincar": [110, 121, 134, 98, 126, 102], "acrobot": [367, 469, 406, 497]}[env]
    assert [a.R0 for a in agents] == want
    return agents


def device():
    import torch
    return torch.device("cuda", 0)


def upload(agents, with_uidx=False, maxR=None):
    """One batch [E][nant+1][maxR], maxR = max R0 + 8 rounded even; SENTINEL beyond every agent's rules.
    Returns (Problem, rant [E][nant][maxR], host copies of rb / rant / uidx)."""
    import torch
    dev = device()
    f = agents[0].fr.five
    nant, E = f.nant, len(agents)
    maxR = maxR or (max(a.R0 for a in agents) + 8 + 1) // 2 * 2
    rb = np.full((E, nant + 1, maxR), SENTINEL)
    rant = np.full((E, nant, maxR), SENTINEL)
    uidx = np.full((E, nant, maxR), 3, dtype=np.int16)      # a valid universe index
    for e, a in enumerate(agents):
        rb[e, :nant, : a.R0], rb[e, nant, : a.R0] = a.veval, a.rconc
        rant[e, :, : a.R0] = a.rant.T
        uidx[e, :, : a.R0] = a.uidx
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    prob = frirl_amd.Problem(t(np.array(f.u)), t(np.array(f.ve)), t(rb), t(np.array([a.R0 for a in agents], dtype=np.int32)),
                             t(uidx) if with_uidx else None)
    return prob, t(rant), (rb, rant, uidx)


def agent_for(env, start=None):
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), device())
    if start is not None:
        for k, v in enumerate(start):
            agent.desc.values_def[k] = float(v)
    return agent


@functools.lru_cache(maxsize=None)
def single_path(env, e, strategy):
    """frirl_hip_reduce_shared on a copy of agent e's slab with agent.values_def = its start state: (kept, result fields)"""
    import torch
    a = case(env)[e]
    prob, rant, _ = upload([a])
    kept, res = prob.reduce_shared(agent_for(env, a.start), strategy, 0.0, 0, rant=rant[0])
    torch.cuda.synchronize()
    return kept.copy(), (res.rules_before, res.rules_after, res.steps_incremental, res.reward)


def starts_tensor(agents):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack([a.start for a in agents]))).to(device())


def check_agent(env, agents, e, strategy, depth_used, kept, res, prob, rant_d, host, with_uidx, oracle=True, case_index=None):
    """Agent e after a call: the oracle, the single-base path, the device state (case_index: its index in case(env) where that is not e)."""
    a = agents[e]
    rb0, rant0, uidx0 = host
    nant, R0, R1 = a.veval.shape[0], a.R0, res.rules_after
    assert res.rules_before == R0 and R1 == len(kept) and (np.diff(kept) > 0).all()
    if oracle:                                                       # 1. the oracle's sequential reduction from the same start state
        want_rant, want_rconc = a.reduced(strategy)
        assert R1 == len(want_rconc), (e, R1, len(want_rconc))
        assert (a.rant[kept] == want_rant).all() and (a.rconc[kept] == want_rconc).all(), f"agent {e}: surviving rules / order"
    if env is not None:                                              # 2. the single-base path
        k1, (before, after, steps_inc, reward) = single_path(env, e if case_index is None else case_index, strategy)
        assert (before, after) == (R0, R1) and (k1 == kept).all(), (e, after, R1)
        assert res.steps_incremental == steps_inc and res.reward == reward
    assert res.rounds == -(-R0 // depth_used), (e, res.rounds, R0, depth_used)
    # 3. device state: compacted columns, zeroed tail, everything beyond the agent's rules untouched
    rb = prob.rb[e].cpu().numpy()
    assert int(prob.nrules[e]) == R1
    assert (rb[:nant, :R1] == a.veval[:, kept]).all() and (rb[nant, :R1] == a.rconc[kept]).all()
    assert (rb[:, R1:R0] == 0).all() and (rb[:, R0:] == rb0[e][:, R0:]).all()
    ra = rant_d[e].cpu().numpy()
    assert (ra[:, :R1] == a.rant[kept].T).all() and (ra[:, R1:R0] == 0).all() and (ra[:, R0:] == rant0[e][:, R0:]).all()
    if with_uidx:
        ui = prob.uidx[e].cpu().numpy()
        assert (ui[:, :R1] == a.uidx[:, kept]).all() and (ui[:, R1:R0] == 0).all() and (ui[:, R0:] == uidx0[e][:, R0:]).all()


def run_batch(env, agents, strategy, depth, with_uidx=False, active=None):
    import torch
    prob, rant_d, host = upload(agents, with_uidx)
    act = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to(device())
    kept, res = prob.reduce_batch(agent_for(env), strategy, 0.0, depth, rant=rant_d, start_states=starts_tensor(agents), active=act)
    torch.cuda.synchronize()
    return kept, res, prob, rant_d, host


def depth_used(depth, E, A=3):
    return depth or frirl_amd.lib().frirl_hip_reduce_batch_depth(E, A)


@pytest.mark.parametrize("strategy,with_uidx", [(1, True), (2, False)])
def test_mountaincar_batch_equals_sequential_reduction_per_agent(strategy, with_uidx):
    """E = 6 agents with R0 = 110 ... 134 and different start states; depths 0, 3 and 1 keep identical sets (invariance)."""
    agents = case("mountaincar")
    want = {1: [28, 25, 23, 23, 48, 17], 2: [52, 31, 26, 15, 33, 24]}[strategy]
    first = None
    for depth in (0, 3, 1):
        kept, res, prob, rant_d, host = run_batch("mountaincar", agents, strategy, depth, with_uidx)
        assert [r.rules_after for r in res] == want
        for e in range(len(agents)):
            check_agent("mountaincar", agents, e, strategy, depth_used(depth, 6), kept[e], res[e], prob, rant_d, host, with_uidx)
        if first is None:
            first = kept
        assert all((k == k0).all() for k, k0 in zip(kept, first)), depth
        assert len({r.rounds for r in res}) > 1 or depth == 0, "the agents were meant to finish after different numbers of rounds"


@pytest.mark.parametrize("strategy,depth", [(1, 0), (2, 5)])
def test_acrobot_batch_with_ragged_rounds_and_a_rejecting_agent(strategy, depth):
    """R0 = 367, 469, 406, 497; agent 3's baseline reward (-160) is not good, so every one of its candidates is rejected."""
    agents = case("acrobot")
    kept, res, prob, rant_d, host = run_batch("acrobot", agents, strategy, depth)
    assert [r.rules_after for r in res] == {1: [182, 37, 310, 497], 2: [155, 194, 196, 497]}[strategy]
    assert res[3].reward == -160.0 and (kept[3] == np.arange(497)).all()
    for e in range(4):
        check_agent("acrobot", agents, e, strategy, depth_used(depth, 4), kept[e], res[e], prob, rant_d, host, False)


def test_cartpole_one_rule_base_two_start_states():
    """21 actions (8 lanes per row, three passes of 4 conclusions): the default agent's rule base twice, reduced from two start states."""
    agents = case("cartpole")
    assert agents[0].baseline() != agents[1].baseline()
    kept, res, prob, rant_d, host = run_batch("cartpole", agents, 1, 0)
    for e in range(2):
        check_agent("cartpole", agents, e, 1, depth_used(0, 2, 21), kept[e], res[e], prob, rant_d, host, False)
    assert res[0].steps_incremental != res[1].steps_incremental or res[0].reward != res[1].reward


def test_inactive_agents_are_untouched():
    """Agents 1 and 4 switched off: slabs and nrules bit-identical afterwards, rules_before == rules_after; the others as before."""
    agents = case("mountaincar")
    active = [1, 0, 1, 1, 0, 1]
    kept, res, prob, rant_d, host = run_batch("mountaincar", agents, 1, 3, with_uidx=True, active=active)
    rb0, rant0, uidx0 = host
    for e in range(6):
        if active[e]:
            check_agent("mountaincar", agents, e, 1, 3, kept[e], res[e], prob, rant_d, host, True)
            continue
        assert (prob.rb[e].cpu().numpy() == rb0[e]).all() and (rant_d[e].cpu().numpy() == rant0[e]).all() and (prob.uidx[e].cpu().numpy() == uidx0[e]).all()
        assert int(prob.nrules[e]) == agents[e].R0 == res[e].rules_before == res[e].rules_after
        assert res[e].rounds == 0 and res[e].rollouts == 0 and (kept[e] == np.arange(agents[e].R0)).all()


def test_one_agent_equals_the_single_base_path():
    """E = 1: the same kept set, counters and device state as frirl_hip_reduce_shared at the same depth."""
    import torch
    a = case("mountaincar")[2]
    prob1, rant1, _ = upload([a])
    k1, r1 = prob1.reduce_shared(agent_for("mountaincar", a.start), 2, 0.0, 7, rant=rant1[0])
    torch.cuda.synchronize()
    kept, res, prob, rant_d, host = run_batch("mountaincar", [a], 2, 7)
    assert (kept[0] == k1).all()
    for f in ("rules_before", "rules_after", "rounds", "rollouts", "steps_incremental", "reward"):
        assert getattr(res[0], f) == getattr(r1, f), f
    assert (prob.rb.cpu().numpy() == prob1.rb.cpu().numpy()).all() and (rant_d.cpu().numpy() == rant1.cpu().numpy()).all()
    check_agent(None, [a], 0, 2, 7, kept[0], res[0], prob, rant_d, host, False)


def test_tiny_rule_base_next_to_a_normal_one():
    """An agent with 4 rules (the corner rule base cut to R0 < depth: a single round whose tree has 2^4 - 1 nodes) beside a
    110-rule agent."""
    import torch
    normal = case("mountaincar")[0]
    fr = ob.Frirl("mountaincar", trig_mode=1)                         # untrained: the 2^3 corner rules
    assert fr.five.R == 8
    tiny = Trained("mountaincar", normal.start, rules=(np.array(fr.five.rant[:4]), np.array(fr.five.rconc[:4])))
    agents = [tiny, normal]
    prob1, rant1, _ = upload([tiny])
    k1, r1 = prob1.reduce_shared(agent_for("mountaincar", tiny.start), 1, 0.0, 6, rant=rant1[0])
    torch.cuda.synchronize()
    kept, res, prob, rant_d, host = run_batch("mountaincar", agents, 1, 6)
    assert res[0].rounds == 1 and res[0].rollouts == 1 + 15 == r1.rollouts and (kept[0] == k1).all() and res[0].rules_after == r1.rules_after
    assert res[0].steps_incremental == r1.steps_incremental and res[0].reward == r1.reward
    check_agent(None, agents, 0, 1, 6, kept[0], res[0], prob, rant_d, host, False)
    check_agent("mountaincar", agents, 1, 1, 6, kept[1], res[1], prob, rant_d, host, False, case_index=0)


class BatchDesc(C.Structure):
    """struct frirl_hip_batch_desc (include/frirl_hip.h)."""
    _fields_ = [("nant", C.c_int32), ("U", C.c_int32), ("E", C.c_int32), ("maxR", C.c_int32), ("u", C.c_void_p), ("ve", C.c_void_p),
                ("agent", frirl_amd.AgentDesc), ("R0", C.c_int32), ("rant0", C.c_void_p), ("rconc0", C.c_void_p), ("start_states", C.c_void_p),
                ("device_select", C.c_int32), ("device", C.c_int32)]


def test_batch_object_reduces_every_agent_from_its_own_start_state():
    """frirl_hip_batch_reduce_all: six mountaincar agents trained on the device from desc.start_states; every agent's reduced rule
    base equals the oracle's reduction of that agent's own learned rule base (downloaded before the reduction) from its start state."""
    L = frirl_amd.lib()
    d = frirl_amd.demo_describe("mountaincar")
    nant, E, maxR = d["nant"], 6, 512
    start = np.ascontiguousarray(np.stack([a.start for a in case("mountaincar")]))
    grid = np.zeros((nant, frirl_amd.MAX_GRID))
    for k, g in enumerate(d["grids"]):
        grid[k, : len(g)] = g
    ncorner = 2 ** nant
    rant0 = np.zeros((ncorner, nant))
    for k in range(nant):
        div = ncorner >> (k + 1)
        rant0[:, k] = [d["grids"][k].min() if ((j // div) % 2) == 0 else d["grids"][k].max() for j in range(ncorner)]
    rconc0 = np.zeros(ncorner)
    u, ve, ave = np.ascontiguousarray(d["u"]), np.ascontiguousarray(d["ve"]), np.ascontiguousarray(d["action_ve"])
    desc = BatchDesc()
    desc.nant, desc.U, desc.E, desc.maxR, desc.u, desc.ve = nant, d["U"], E, maxR, u.ctypes.data, ve.ctypes.data
    desc.R0, desc.rant0, desc.rconc0, desc.start_states = ncorner, rant0.ctypes.data, rconc0.ctypes.data, start.ctypes.data
    ag = desc.agent
    ag.alpha, ag.gamma, ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"]
    ag.weight_significant, ag.skip_rules, ag.A, ag.env_kind, ag.max_steps, ag.no_random = d["weight_thr"], d["skip_rules"], d["A"], d["kind"], d["max_steps"], 1
    ag.reward_good_above, ag.qdiff_final_tolerance = d["reward_good_above"], d["qdiff_final_tolerance"]
    for k in range(nant):
        ag.grid_len[k], ag.grid_div[k], ag.values_def[k] = len(d["grids"][k]), d["grid_div"][k], d["values_def"][k]
    ag.grid_values, ag.action_ve = grid.ctypes.data, ave.ctypes.data
    b = L.frirl_hip_batch_create(C.byref(desc))
    assert b, L.frirl_hip_last_error()
    try:
        episodes = C.c_int32()
        frirl_amd.check(L.frirl_hip_batch_train(b, 1000, C.byref(episodes)), "frirl_hip_batch_train")

        def download(e):
            R = C.c_int32()
            rant, rconc = np.zeros((maxR, nant)), np.zeros(maxR)
            dp = C.POINTER(C.c_double)
            frirl_amd.check(L.frirl_hip_batch_get_rulebase(b, e, C.byref(R), rant.ctypes.data_as(dp), rconc.ctypes.data_as(dp)), "frirl_hip_batch_get_rulebase")
            return rant[: R.value].copy(), rconc[: R.value].copy()

        before = [download(e) for e in range(E)]
        assert len({len(q) for _, q in before}) > 1, "the start states were meant to give different rule bases"
        res = (frirl_amd.ReduceResult * E)()
        reduced = C.c_int32(-1)
        frirl_amd.check(L.frirl_hip_batch_reduce_all(b, 1, 0.0, 0, res, C.byref(reduced)), "frirl_hip_batch_reduce_all")
        assert reduced.value == sum(r.rules_after < r.rules_before for r in res) > 0
        for e in range(E):
            rant, rconc = download(e)
            orc = Trained("mountaincar", start[e], rules=before[e])
            want_rant, want_rconc = orc.reduced(1)
            assert res[e].rules_before == len(before[e][1]) and res[e].rules_after == len(rconc) == len(want_rconc), (e, len(rconc), len(want_rconc))
            assert (rant == want_rant).all() and (rconc == want_rconc).all(), f"agent {e}"
    finally:
        L.frirl_hip_batch_destroy(b)
