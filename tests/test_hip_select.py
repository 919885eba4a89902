"""Selection inside a population on the device (csrc/clone.hip and the frirl_hip_batch_clone / _select calls of csrc/batch.hip).

1. frirl_hip_clone_agents against tests/select_ref.py::clone_ref, byte for byte, every array inside a larger tensor with sentinels
2. the batch object against the oracle chains of tests/select_cases.py (asserted on the CPU by tests/test_select_ref.py)
3. frirl_hip_batch_select equals frirl_hip_batch_evaluate + frirl_hip_select_plan + frirl_hip_batch_clone on a twin batch
4. refusals leave the batch as it was; frirl_demo --select

The batch object is opaque: its state is read through frirl_hip_batch_agent_report, _get_rulebase, _get_hparams and _get_exploration,
and what those do not show (sticky flag, index mirror, spread state) through the episodes trained afterwards, which read all three.
Bars: counters, reward bits, antecedents exact; consequents <= 1e-9 relative against the oracle (the bar of the other rows tests).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import hparam_rows_cases as rc
from tests import hparams_cases as hc
from tests import select_cases as sc
from tests.select_ref import BAD_RULES, BAD_SRC, CHAINED, CLONED, KEPT, clone_ref, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
E7 = 7
PAD = 64                    # sentinel bytes on either side of every array (a multiple of 16: the rows stay aligned)
SENTINEL = 0xA5
I32 = C.POINTER(C.c_int32)


# ---- 1. the primitive ----------------------------------------------------------------------------------------------------------------
def random_state(nant, maxR, rng, E=E7):
    """Every array of the contract for 7 agents, filled with noise also beyond the rule counts; nrules: a source with 1 rule (0) and
    one with maxR (1), destinations with more (2) and fewer (3) rules than those, the counts 0 (4) and maxR + 1 (5), a middling one (6).
    Another E: counts drawn from 0 .. maxR + 1."""
    n, M = nant, maxR
    counts = [1, M, min(M, 5), 1, 0, M + 1, max(1, M // 2)] if E == E7 else rng.integers(0, M + 2, size=E)
    f = lambda *shape: rng.normal(size=shape)
    i = lambda *shape: rng.integers(-5, 50, size=shape).astype(np.int32)
    return dict(
        rb=f(E, n + 1, M), nrules=np.array(counts, dtype=np.int32),
        uidx=rng.integers(0, 65536, size=(E, n, M)).astype(np.uint16), rant=f(E, n, M), fus=i(E), spread_ant=f(E, n), spread_R=i(E),
        states=f(E, n - 1), q_ant=f(E, n), done=i(E), ep_steps=i(E), ep_reward=f(E), status=i(E), start_states=f(E, n - 1), episode=i(E),
        prev_nrules=rng.integers(0, M + 2, size=E).astype(np.int32), prev_steps=i(E), prev_reward=f(E), prev_rconc=f(E, M), converged=i(E), episodes=i(E),
        epended=i(E), weights=f(E, M))


# fan-out of source 0 to three destinations with more / no / too many rules of their own and source 1 to one with fewer; every way of
# being refused (-1, E, a source with 0 and with maxR + 1 rules, a source that is itself replaced); a chained pair beside a valid clone
SRC_TABLES = [[0, 1, 0, 1, 0, 0, 6], [-1, 7, 4, 5, 4, 5, 2], [1, 0, 6, 3, 4, 5, 6]]
STATUS = [[KEPT, KEPT, CLONED, CLONED, CLONED, CLONED, KEPT], [BAD_SRC, BAD_SRC, BAD_RULES, BAD_RULES, KEPT, KEPT, CHAINED],
          [CHAINED, CHAINED, CLONED, KEPT, KEPT, KEPT, KEPT]]
ENVS_FIELDS = [k for k, _ in frirl_amd.EnvsDesc._fields_]
CONV_FIELDS = [k for k, _ in frirl_amd.ConvergenceDesc._fields_]


class Embedded:
    """The arrays of a state on the device, each in the middle of its own byte tensor between two runs of sentinel bytes."""

    def __init__(self, state, absent=(), pad=None):
        import torch
        self.names = [k for k in state if k not in absent]
        self.pad = dict(pad or {})
        self.buf, self.size = {}, {}
        for k in self.names + ["src", "out_status"]:
            nbytes = state[k].nbytes if k in state else 4 * len(state["nrules"])
            self.size[k] = nbytes
            p = self.pad.get(k, PAD)
            host = np.full(p + nbytes + PAD, SENTINEL, dtype=np.uint8)
            if k in state:
                host[p: p + nbytes] = np.frombuffer(state[k].tobytes(), dtype=np.uint8)
            self.buf[k] = torch.from_numpy(host).to(DEV)

    def ptr(self, k):
        return self.buf[k].data_ptr() + self.pad.get(k, PAD) if k in self.buf else None

    def set(self, k, array):
        import torch
        p = self.pad.get(k, PAD)
        self.buf[k][p: p + array.nbytes] = torch.from_numpy(np.frombuffer(array.tobytes(), dtype=np.uint8).copy()).to(DEV)

    def get(self, k, like):
        p = self.pad.get(k, PAD)
        host = self.buf[k].cpu().numpy()
        assert (host[:p] == SENTINEL).all() and (host[p + self.size[k]:] == SENTINEL).all(), f"{k}: a sentinel was overwritten"
        return np.frombuffer(host[p: p + self.size[k]].tobytes(), dtype=like.dtype).reshape(like.shape)


def run_clone(state, src, absent=(), no_envs=False, no_status=False, pad=None):
    """frirl_hip_clone_agents on an embedded copy of `state`; returns (state afterwards, status or None)."""
    import torch
    em = Embedded(state, absent, pad)
    em.set("src", np.array(src, dtype=np.int32))
    E, n1, M = state["rb"].shape
    bases = frirl_amd.RuleBases(E, M, em.ptr("rb"), em.ptr("nrules"), em.ptr("uidx"))
    envs = frirl_amd.EnvsDesc(*[em.ptr(k) for k in ENVS_FIELDS])
    has_conv = "prev_rconc" not in absent
    conv = frirl_amd.ConvergenceDesc(*[em.ptr(k) for k in CONV_FIELDS])
    rc_ = frirl_amd.lib().frirl_hip_clone_agents(C.byref(bases), n1 - 1, None if no_envs else C.byref(envs), C.byref(conv) if has_conv else None,
                                                 em.ptr("weights"), em.ptr("src"), None if no_status else em.ptr("out_status"), None)
    frirl_amd.check(rc_, "frirl_hip_clone_agents")
    torch.cuda.synchronize()
    after = {k: em.get(k, state[k]) for k in em.names}
    status = em.get("out_status", np.zeros(E, dtype=np.int32))
    assert (em.get("src", np.zeros(E, dtype=np.int32)) == np.array(src)).all()
    if no_status:
        assert (status.view(np.uint8) == SENTINEL).all()
    return after, None if no_status else status


def assert_state_equal(got, want, where):
    assert set(got) == set(k for k, v in want.items() if v is not None), where
    for k, v in got.items():
        assert v.tobytes() == want[k].tobytes(), (where, k, np.argwhere(v != want[k])[:4].tolist())


@pytest.mark.parametrize("maxR", [2, 6, 16, 258, 512, 1030])
@pytest.mark.parametrize("nant", [2, 3, 5, 8])
def test_clone_agents_matches_the_contract_byte_for_byte(nant, maxR):
    """maxR 2 (the minimum), 6 (index rows not 16-byte aligned), 16 and 512 (aligned: the 16-byte index path), 258 (a 256-chunk and a
    remainder of 2), 1030; three src tables each.  Every array of every agent, the untouched ones included, and status."""
    state = random_state(nant, maxR, np.random.default_rng(1000 * nant + maxR))
    for t, (src, expect) in enumerate(zip(SRC_TABLES, STATUS)):
        want, st = clone_ref(state, src)
        assert st.tolist() == expect
        got, status = run_clone(state, src)
        assert status.tolist() == expect, (t, status.tolist())
        assert_state_equal(got, want, (nant, maxR, t))
        if t == 0:          # the invariant, on rows that were zero beyond their counts to begin with
            tidy = {k: v.copy() for k, v in state.items()}
            for e in range(E7):
                R = min(max(int(state["nrules"][e]), 0), maxR)
                for k in ("rb", "rant", "uidx", "prev_rconc", "weights"):
                    tidy[k][e][..., R:] = 0
                tidy["prev_nrules"][e] = R
            got, _ = run_clone(tidy, src)
            for e in range(E7):
                for k in ("rb", "rant", "uidx", "prev_rconc"):
                    assert not got[k][e][..., int(got["nrules"][e]) if expect[e] == CLONED else maxR:].any(), (k, e)


@pytest.mark.parametrize("absent", [("uidx",), ("rant",), ("weights",), ("prev_nrules", "prev_steps", "prev_reward", "prev_rconc", "converged", "episodes", "epended"),
                                    ("epended",), "status", "envs"], ids=["uidx", "rant", "weights", "conv", "epended", "status", "envs"])
@pytest.mark.parametrize("nant,maxR", [(3, 258), (5, 6), (2, 16)])
def test_clone_agents_with_optional_arrays_absent(nant, maxR, absent):
    state = random_state(nant, maxR, np.random.default_rng(7 * nant + maxR))
    src = SRC_TABLES[0]
    if absent == "status":
        got, _ = run_clone(state, src, no_status=True)
        want, _ = clone_ref(state, src)
    elif absent == "envs":
        got, status = run_clone(state, src, no_envs=True)
        want, st = clone_ref({k: (None if k in ENVS_FIELDS else v) for k, v in state.items()}, src)
        want = {k: (state[k] if k in ENVS_FIELDS else v) for k, v in want.items()}          # the arrays exist, the call is not shown them
        assert status.tolist() == st.tolist()
    else:
        got, status = run_clone(state, src, absent=absent)
        want, st = clone_ref({k: (None if k in absent else v) for k, v in state.items()}, src)
        assert status.tolist() == st.tolist()
    assert_state_equal(got, want, (nant, maxR, absent))


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_an_index_mirror_off_the_16_byte_grid_takes_the_narrow_path(offset):
    """maxR % 8 == 0 but the mirror starts 4, 8 or 12 bytes past a 16-byte boundary: the rows are not aligned and must not be assumed to be."""
    state = random_state(3, 16, np.random.default_rng(offset))
    want, _ = clone_ref(state, SRC_TABLES[0])
    got, _ = run_clone(state, SRC_TABLES[0], pad=dict(uidx=PAD + offset))
    assert_state_equal(got, want, offset)


@pytest.mark.parametrize("E,nant,maxR", [(2047, 2, 6), (2048, 3, 8), (6149, 2, 6), (16411, 3, 16), (65536 + 3, 2, 2)])
def test_clone_agents_on_large_batches(E, nant, maxR):
    """Below 2048 agents a destination is shared by several workgroups where its slab gives them work, from 2048 on it has one: 2047,
    2048, and up to 65539 agents (more than a grid dimension of 65535 holds).  A random src table: a third of the agents are sources,
    the others take a random agent, a source or not (chains), or an index outside the batch; counts 0 .. maxR + 1."""
    rng = np.random.default_rng(E)
    state = random_state(nant, maxR, rng, E=E)
    src = np.arange(E)
    dest = rng.random(E) > 1 / 3
    src[dest] = rng.integers(-2, E + 2, size=int(dest.sum()))
    src[np.nonzero(dest)[0][:2]] = (-1, E)
    want, st = clone_ref(state, src)
    assert all((st == k).sum() > E // 200 for k in (KEPT, CLONED, CHAINED, BAD_RULES)) and (st == BAD_SRC).any()
    got, status = run_clone(state, src.tolist())
    assert (status == st).all()
    assert_state_equal(got, want, (E, nant, maxR))


def test_clone_agents_refuses_bad_arguments_on_the_device_too():
    state = random_state(3, 6, np.random.default_rng(3))
    em = Embedded(state)
    em.set("src", np.array(SRC_TABLES[0], dtype=np.int32))
    lib = frirl_amd.lib()
    for E, M, nant, rb, src in ((0, 6, 3, "rb", "src"), (E7, 5, 3, "rb", "src"), (E7, 6, 1, "rb", "src"), (E7, 6, 10, "rb", "src"), (E7, 6, 3, None, "src"),
                                (E7, 6, 3, "rb", None)):
        bases = frirl_amd.RuleBases(E, M, em.ptr(rb) if rb else None, em.ptr("nrules"), em.ptr("uidx"))
        assert lib.frirl_hip_clone_agents(C.byref(bases), nant, None, None, None, em.ptr(src) if src else None, None, None) == -2
    for k in em.names:
        assert em.get(k, state[k]).tobytes() == state[k].tobytes()


def test_problem_clone_agents_marks_the_packed_mirrors_stale():
    """Problem.clone_agents on a trained mountaincar batch against clone_ref, and the packed index mirror and codes are repacked before
    the next scan: the clone's rule distances are its source's."""
    import torch
    E = 6
    prob, agent, envs = frirl_amd.demo_fresh_batch("mountaincar", E, 512, DEV)
    rows = frirl_amd.HparamRows(E, DEV, weight_significant=[0.05, 0.002, 0.05, 0.3, 0.002, 0.05])
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=5, rows=rows)
    conv = run.conv
    torch.cuda.synchronize()
    assert len(set(prob.nrules.tolist())) > 1
    assert prob.pidx is not None
    prob.rule_distance(envs.rant[:, :, 3].contiguous())
    assert prob._pidx_key is not None
    grab = lambda: dict(rb=prob.rb, nrules=prob.nrules, uidx=prob.uidx, rant=envs.rant, fus=envs.fus,
                        spread_ant=envs.spread_ant, spread_R=envs.spread_R, states=envs.states, q_ant=envs.q_ant, done=envs.done, ep_steps=envs.ep_steps,
                        ep_reward=envs.ep_reward, status=envs.status, episode=envs.episode, prev_nrules=conv.prev_nrules, prev_steps=conv.prev_steps,
                        prev_reward=conv.prev_reward, prev_rconc=conv.prev_rconc, converged=conv.converged, episodes=conv.episodes, epended=conv.epended)
    before = {k: v.cpu().numpy().copy() for k, v in grab().items()}
    src = [0, 1, 1, 3, 0, 1]
    status = prob.clone_agents(envs, torch.tensor(src, dtype=torch.int32, device=DEV), conv=conv)
    assert prob._pidx_key is None and prob._codes_key is None
    torch.cuda.synchronize()
    want, st = clone_ref(before, src)
    assert status.tolist() == st.tolist() == [KEPT, KEPT, CLONED, KEPT, CLONED, CLONED]
    after = {k: v.cpu().numpy() for k, v in grab().items()}
    assert_state_equal(after, want, "trained batch")
    d, hit = prob.rule_distance(envs.rant[:, :, 3].contiguous())          # rule 3 of every agent, the clones' being their sources'
    torch.cuda.synchronize()
    assert hit.tolist() == [3] * E
    for e in (2, 4, 5):
        R = int(prob.nrules[e])
        assert torch.equal(d[e, :R], d[src[e], :R]), e


# ---- 2. the batch object against the oracle chains ---------------------------------------------------------------------------------------
def train(batch, max_episodes):
    ran = C.c_int32(0)
    frirl_amd.check(frirl_amd.lib().frirl_hip_batch_train(batch, max_episodes, C.byref(ran)), "frirl_hip_batch_train")
    return ran.value


def rulebase(batch, e, nant):
    R = C.c_int32(0)
    lib = frirl_amd.lib()
    frirl_amd.check(lib.frirl_hip_batch_get_rulebase(batch, e, C.byref(R), None, None), "frirl_hip_batch_get_rulebase")
    rant, rconc = np.zeros((R.value, nant)), np.zeros(R.value)
    frirl_amd.check(lib.frirl_hip_batch_get_rulebase(batch, e, C.byref(R), rant.ctypes.data_as(frirl_amd._DP), rconc.ctypes.data_as(frirl_amd._DP)), "frirl_hip_batch_get_rulebase")
    return rant, rconc


def batch_state(batch, E, nant):
    """Everything the getters show, as bytes per key."""
    out = {k: v.tobytes() for k, v in frirl_amd.batch_agent_report(batch).items()}
    out.update({"hp_" + k: v.tobytes() for k, v in frirl_amd.batch_get_hparams(batch).items()})
    out.update({"ex_" + k: v.tobytes() for k, v in frirl_amd.batch_get_exploration(batch).items()})
    for e in range(E):
        rant, rconc = rulebase(batch, e, nant)
        out[f"rant{e}"], out[f"rconc{e}"] = rant.tobytes(), rconc.tobytes()
    return out


def check_batch_agent(batch, rep, e, run, episodes, where):
    fr = run["fr"]
    f = fr.five
    got = (int(rep["converged"][e]), int(rep["episodes"][e]), int(rep["rules"][e]), int(rep["ep_steps"][e]))
    assert got == (0, episodes, f.R, fr.ep_steps), (where, e, got, (f.R, fr.ep_steps))
    assert rep["ep_reward"][e].view(np.uint64) == np.float64(fr.ep_reward).view(np.uint64), (where, e)
    rant, rconc = rulebase(batch, e, f.nant)
    assert (rant == np.array(f.rant[: f.R])).all(), (where, e, "antecedents / rule order")
    ref = np.array(f.rconc[: f.R])
    assert (np.abs(rconc - ref) <= TOL * np.maximum(np.abs(ref), 1e-9)).all(), (where, e, "consequents")


@pytest.mark.parametrize("inherit", [0, 1])
@pytest.mark.parametrize("env", sc.ENVS)
def test_batch_clone_follows_the_oracle_chains(env, inherit):
    """One agent per role -- per case a source under set a and its clone-to-be under set b, and an agent nobody clones -- all greedy from
    the demo's start state: frirl_hip_batch_set_hparams, train k episodes, frirl_hip_batch_clone, train m more.  inherit_rows = 0: the
    clone ends where the oracle's chain a -> b ends; 1: byte for byte where its source ends, under the source's row."""
    cases = sc.env_cases(env)
    k, m = sc.EPISODES[env]
    names = [n for c in cases for n in (c[1], c[2])] + [sc.UNTOUCHED[env]]
    E = len(names)
    nant = frirl_amd.demo_describe(env)["nant"]
    src = list(range(E))
    for i in range(len(cases)):
        src[2 * i + 1] = 2 * i
    columns = rc.columns([hc.demo_desc(env, n) for n in names])
    batch = frirl_amd.demo_batch_object(env, E, sc.MAXR)
    try:
        frirl_amd.batch_set_hparams(batch, **columns)
        assert train(batch, k + 1) == k
        before = frirl_amd.batch_agent_report(batch)
        assert frirl_amd.batch_clone(batch, src, inherit_rows=bool(inherit)) == len(cases)
        rep = frirl_amd.batch_agent_report(batch)
        hp = frirl_amd.batch_get_hparams(batch)
        for e in range(E):          # straight after the clone: the source's rule count, the agent's own episode counter, no last episode
            assert rep["rules"][e] == before["rules"][src[e]] and rep["episodes"][e] == k and rep["converged"][e] == 0
            assert rep["ep_steps"][e] == (before["ep_steps"][e] if src[e] == e else -1)
            for col, v in hp.items():
                assert v[e] == columns[col][src[e] if inherit else e], (col, e)
        assert train(batch, m + 1) == m
        rep = frirl_amd.batch_agent_report(batch)
        for i, (_, a, b, _, _) in enumerate(cases):
            check_batch_agent(batch, rep, 2 * i, sc.chain(env, a, a, k, m), k + m, (env, a, "source"))
            check_batch_agent(batch, rep, 2 * i + 1, sc.chain(env, a, a if inherit else b, k, m), k + m, (env, a, b, "clone"))
            if inherit:
                s, c = rulebase(batch, 2 * i, nant), rulebase(batch, 2 * i + 1, nant)
                assert s[0].tobytes() == c[0].tobytes() and s[1].tobytes() == c[1].tobytes(), (env, a, "the clone left its source")
                assert all(rep[key][2 * i] == rep[key][2 * i + 1] for key in rep)
        check_batch_agent(batch, rep, E - 1, sc.chain(env, names[-1], names[-1], k, m), k + m, (env, "untouched"))
    finally:
        frirl_amd.lib().frirl_hip_batch_destroy(batch)


def test_batch_clone_inherits_exploration_rows_and_leaves_unset_columns_unset():
    """Exploration rows and a single hyper-parameter column set: with inherit_rows the clones read their sources' epsilon, horizon and
    alpha; the unset columns still answer with the batch's own value for everybody; without it nothing moves."""
    env, E = "mountaincar", 6
    d = frirl_amd.demo_describe(env)
    eps, hor, alpha = np.linspace(0.0, 0.5, E), np.arange(E, dtype=np.int32) + 3, np.linspace(0.1, 0.6, E)
    src = [0, 0, 2, 2, 4, 0]
    batch = frirl_amd.demo_batch_object(env, E, 512, seed=5)
    try:
        frirl_amd.batch_set_exploration(batch, epsilon=eps, horizon=hor)
        frirl_amd.batch_set_hparams(batch, alpha=alpha)
        train(batch, 3)
        assert frirl_amd.batch_clone(batch, src, inherit_rows=False) == 3
        ex, hp = frirl_amd.batch_get_exploration(batch), frirl_amd.batch_get_hparams(batch)
        assert (ex["epsilon"] == eps).all() and (ex["horizon"] == hor).all() and (hp["alpha"] == alpha).all()
        assert frirl_amd.batch_clone(batch, src, inherit_rows=True) == 3
        ex, hp = frirl_amd.batch_get_exploration(batch), frirl_amd.batch_get_hparams(batch)
        assert (ex["epsilon"] == eps[src]).all() and (ex["horizon"] == hor[src]).all() and (hp["alpha"] == alpha[src]).all()
        assert (hp["gamma"] == d["gamma"]).all() and (hp["skip_rules"] == d["skip_rules"]).all() and (hp["weight_significant"] == d["weight_thr"]).all()
        frirl_amd.batch_set_exploration(batch, horizon_all=9, epsilon=eps)
        assert (frirl_amd.batch_get_exploration(batch)["horizon"] == 9).all()
        train(batch, 3)             # rows set, clones in place: training simply goes on
        assert (frirl_amd.batch_agent_report(batch)["episodes"] == 4).all()
    finally:
        frirl_amd.lib().frirl_hip_batch_destroy(batch)


# ---- 3. select equals its parts --------------------------------------------------------------------------------------------------------
def select_batch(E):
    """Mountaincar agents that differ in start state and hyper-parameter set, 12 episodes in."""
    env = "mountaincar"
    d = frirl_amd.demo_describe(env)
    rng = np.random.default_rng(4)
    start = np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1)
    sets = rc.demo_sets(env)
    batch = frirl_amd.demo_batch_object(env, E, 512, start_states=start)
    frirl_amd.batch_set_hparams(batch, **rc.columns([hc.demo_desc(env, sets[e % len(sets)]) for e in range(E)]))
    train(batch, 13)
    return batch, d


def test_batch_select_is_evaluate_plan_and_clone():
    E, n, parents, replace = 8, 2, 2, 3
    lib = frirl_amd.lib()
    one, d = select_batch(E)
    two, _ = select_batch(E)
    nant = d["nant"]
    try:
        rng = np.random.default_rng(8)
        starts = np.stack([rng.choice(d["grids"][k], (E, n)) for k in range(d["nstates"])], 2)
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        before = frirl_amd.batch_agent_report(one)
        rconc_before = [rulebase(one, e, nant)[1].tobytes() for e in range(E)]
        scores, src, res = frirl_amd.batch_select(one, n, parents, replace, start_states=starts)
        by_hand = (frirl_amd.RolloutScore * E)()
        best = C.c_int32(-1)
        frirl_amd.check(lib.frirl_hip_batch_evaluate(two, n, starts.ctypes.data_as(frirl_amd._DP), by_hand, C.byref(best)), "frirl_hip_batch_evaluate")
        pairs = [(s.successes, s.reward_sum) for s in by_hand]
        assert [(s.successes, s.reward_sum, s.steps_sum) for s in scores] == [(s.successes, s.reward_sum, s.steps_sum) for s in by_hand]
        want_src, rank = plan_ref(pairs, parents, replace)
        psrc, prank = frirl_amd.select_plan(list(by_hand), parents, replace)
        assert src.tolist() == want_src.tolist() == psrc.tolist() and prank.tolist() == rank.tolist()
        assert frirl_amd.batch_clone(two, psrc) == replace
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        replaced = [e for e in range(E) if src[e] != e]
        assert (res.best, res.parents, res.replaced, res.reserved) == (best.value, parents, replace, 0) and rank[0] == best.value and len(replaced) == replace
        assert res.rules_copied == sum(int(before["rules"][src[e]]) for e in replaced)
        after = frirl_amd.batch_agent_report(one)
        for e in replaced:
            assert rulebase(one, e, nant)[1].tobytes() == rulebase(one, int(src[e]), nant)[1].tobytes() and after["rules"][e] == before["rules"][src[e]]
        assert any(rulebase(one, e, nant)[1].tobytes() != rconc_before[e] for e in replaced), "the selection replaced nothing that can be seen"
        train(one, 4), train(two, 4)        # the sticky flag, the index mirror and the spread state are read by these episodes
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
    finally:
        lib.frirl_hip_batch_destroy(one)
        lib.frirl_hip_batch_destroy(two)


# ---- 4. refusals and the demo ----------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_batch_as_it_was():
    E = 5
    lib = frirl_amd.lib()
    batch, d = select_batch(E)
    nant = d["nant"]
    try:
        before = batch_state(batch, E, nant)
        for src, word in (([0, 1, 5, 3, 4], "agent 2"), ([0, -1, 2, 3, 4], "agent 1"), ([1, 2, 2, 3, 4], "agent 0"), ([0, 1, 2, 4, 3], "agent 3")):
            with pytest.raises(frirl_amd.FrirlHipError, match=word):
                frirl_amd.batch_clone(batch, src)
        assert lib.frirl_hip_batch_clone(batch, None, 0, None) == -2 and lib.frirl_hip_batch_clone(None, (C.c_int32 * E)(), 0, None) == -2
        for args, word in (((1, 3, 3), "parents=3"), ((1, 0, 1), "parents=0"), ((1, 1, -1), "replace=-1"), ((0, 1, 1), "n=0")):
            with pytest.raises(frirl_amd.FrirlHipError, match=word):
                frirl_amd.batch_select(batch, *args)
        assert lib.frirl_hip_batch_get_hparams(batch, None) == -2 and lib.frirl_hip_batch_get_exploration(None, None) == -2
        assert batch_state(batch, E, nant) == before
        train(batch, 3)
        twin, _ = select_batch(E)
        try:
            train(twin, 3)
            assert batch_state(batch, E, nant) == batch_state(twin, E, nant), "a refused call left something behind that training read"
        finally:
            lib.frirl_hip_batch_destroy(twin)
    finally:
        lib.frirl_hip_batch_destroy(batch)


DEMO = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")


def test_demo_runs_generations_of_selection(tmp_path):
    env = "mountaincar"
    sets = rc.demo_sets(env)
    f = tmp_path / "f.txt"
    f.write_text("".join(" ".join(repr(float(hc.demo_desc(env, n)[k])) for k in hc.HP_KEYS) + "\n" for n in sets))
    r = subprocess.run([DEMO, "--env", env, "--agents", "8", "--hparams", str(f), "--select", "2", "--select-episodes", "4", "--select-parents", "2",
                        "--select-replace", "3", "--select-inherit", "--evaluate", "2", "--max-episodes", "12"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(f"select {env}: ")]
    assert len(lines) == 2, r.stdout
    for g, line in enumerate(lines):
        m = re.match(rf"select {env}: generation (\d+) best (\d+) successes (\d+) reward (-?[\d.]+) replaced (\d+) rules_copied (\d+)$", line)
        assert m, line
        assert int(m[1]) == g and 0 <= int(m[2]) < 8 and 0 <= int(m[3]) <= 2 and int(m[5]) == 3 and int(m[6]) >= 3 * 2 ** 3
    report = [l for l in r.stdout.splitlines() if l.startswith(f"batch {env}: agents 8 episodes ")]
    assert len(report) == 1 and re.match(rf"batch {env}: agents 8 episodes (\d+) converged (\d+) ", report[0]), r.stdout
    assert int(report[0].split()[5]) == 11


@pytest.mark.parametrize("flags,word", [(["--merge"], "--merge"), (["--gpus", "2"], "--gpus"), (["--evaluate", "1", "--teach-best", "1"], "--teach-best")])
def test_demo_refuses_selection_with_merge_gpus_and_teaching(flags, word, tmp_path):
    r = subprocess.run([DEMO, "--env", "mountaincar", "--agents", "8", "--select", "2", "--select-episodes", "4", "--select-parents", "2", "--select-replace",
                        "3"] + flags, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and f"--select does not go with {word}" in r.stderr, r.stderr
