"""Recorded roll-outs (frirl_hip_rollout_record, csrc/rollout_record.hip) and teaching from the best agent (frirl_hip_batch_teach).

The reference is the oracle driven step by step: a0 = get_best_action(x0), then x, r, ok, q = env_step(av[a], x) and a = get_best_action(q),
the pick going through oracle.binding.e_greedy_pick under exploration.  The rule bases are those of tests/test_hip_reduce_batch.py
(trained by the oracle), the start rows those of tests/test_hip_rollout_batch.py: starts_for.

Every comparison is exact: bits of obs, q_obs and reward, integers otherwise.  tests/test_hip_rollout_batch.py compares these very rows
exactly on an MI355X and records that no arg-max tie was observed, so exactness is a condition the inputs are known to meet.  Where the
taught rule bases are compared with the oracle's replay (6, 7) the bounds are those of tests/test_hip_teach.py: decisions and rule
order exact, consequents within its contract.

1. logs equal the oracle's            5. capacity, logs that are not recorded, guard regions
2. lane shapes agree bit for bit      6. record -> learn on the device, against TaughtMirror.replay
3. K = 1 equals frirl_hip_rollout_batch  7. frirl_hip_batch_teach
4. exploration across episodes        8. frirl_demo --teach-best
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import teach_ref as tr
from tests.test_hip_reduce_batch import BatchDesc, agent_for, case, upload
from tests.test_hip_rollout_batch import BASE, SEED, oracle_rows, same_bits, starts_for, tens
from tests.test_hip_teach import assert_matches_mirrors, within_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7                       # every log array is filled with it before a call; start flags with SENT_U8
SENT_U8 = 249
ARRAYS = ("obs", "q_obs", "action", "reward", "success", "start")
EPS = 0.3


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def oracle_episode(a, av, x0, max_steps, epsilon=0.0, gid=0, episode=0):
    """One episode on Trained `a`: lists of (obs, q_obs, action, reward, success, start) records."""
    fr, A = a.fr, len(av)
    pick = lambda g, step: ob.e_greedy_pick(g, A, epsilon, 0 if epsilon > 0 else 1, SEED, gid, episode, step)
    x = np.array(x0, dtype=np.float64)
    act = pick(fr.get_best_action(x), 0)
    recs = [(x.copy(), np.zeros_like(x), act, 0.0, 0, 1)]
    for s in range(1, max_steps + 1):
        x, r, ok, q = fr.env_step(av[act], x)
        act = pick(fr.get_best_action(q), s)
        recs.append((np.array(x), np.array(q), act, float(r), int(ok), 0))
        if ok == 1:
            break
    return recs


@functools.lru_cache(maxsize=None)
def oracle_logs(env, K, epsilon=0.0):
    """Log e = K episodes of agent e from starts_for(env, K)[e * K + k], exploration keys (BASE + e, k, step): a list of dicts of arrays
    plus ep_steps / ep_reward / ep_success.  Computed once and never modified."""
    agents = case(env)
    d = frirl_amd.demo_describe(env)
    av, ms = d["grids"][-1], d["max_steps"]
    starts = starts_for(env, K)
    out = []
    for e, a in enumerate(agents):
        a.restore(a.rant, a.rconc)
        recs, eps = [], []
        for k in range(K):
            ep = oracle_episode(a, av, starts[e * K + k], ms, epsilon, BASE + e, k)
            total = 0.0
            for rec in ep[1:]:
                total = total + rec[3]
            eps.append((len(ep) - 1, total, ep[-1][4]))
            recs += ep
        log = dict(obs=np.array([r[0] for r in recs]), q_obs=np.array([r[1] for r in recs]), action=np.array([r[2] for r in recs], np.int32),
                   reward=np.array([r[3] for r in recs]), success=np.array([r[4] for r in recs], np.int32), start=np.array([r[5] for r in recs], np.uint8),
                   ep_steps=np.array([x[0] for x in eps], np.int32), ep_reward=np.array([x[1] for x in eps]), ep_success=np.array([x[2] for x in eps], np.int32))
        for v in log.values():
            v.setflags(write=False)
        out.append(log)
    return out


# ---- device side ------------------------------------------------------------------------------------------------------------------
def guarded_log(Q, K, T, ns, guard=2):
    """A RolloutLog over sentinel-filled buffers with `guard` more logs of sentinel behind every array: (log, whole buffers)."""
    import torch
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=DEV)
    G = Q + guard
    whole = dict(obs=full((G, T, ns), torch.float64, SENT), q_obs=full((G, T, ns), torch.float64, SENT), action=full((G, T), torch.int32, SENT),
                 reward=full((G, T), torch.float64, SENT), success=full((G, T), torch.int32, SENT), start=full((G, T), torch.uint8, SENT_U8),
                 length=full((G,), torch.int32, SENT), ep_steps=full((G, K), torch.int32, SENT), ep_reward=full((G, K), torch.float64, SENT),
                 ep_success=full((G, K), torch.int32, SENT))
    return frirl_amd.RolloutLog(*(whole[k][:Q] for k in frirl_amd.RolloutLog.FIELDS)), whole


def record(env, n, K, T, starts, agent=None, prob=None, **kw):
    """One call into guarded buffers; returns host arrays of the Q logs after checking that the guard regions kept the sentinel."""
    import torch
    prob = prob or upload(case(env))[0]
    agent = agent or agent_for(env)
    Q, ns = prob.E * n, prob.nant - 1
    log, whole = guarded_log(Q, K, T, ns)
    s = None if starts is None else tens(np.ascontiguousarray(starts).reshape(Q, K, ns))
    prob.rollout_record(agent, n, K, T, start_states=s, out=log, **kw)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in whole.items()}
    for k, v in host.items():
        assert (v[Q:] == (SENT_U8 if k == "start" else SENT)).all(), f"{k}: written behind the array"
    return {k: v[:Q] for k, v in host.items()}


def untouched(got, q, lo=0):
    """records lo .. T-1 of log q still hold the sentinel"""
    return all((got[k][q, lo:] == (SENT_U8 if k == "start" else SENT)).all() for k in ARRAYS)


def assert_log_equals(got, q, want, where):
    L = len(want["action"])
    assert int(got["length"][q]) == L, (where, int(got["length"][q]), L)
    for k in ("obs", "q_obs", "reward"):
        assert same_bits(got[k][q, :L], want[k]), (where, k)
    for k in ("action", "success", "start"):
        assert (got[k][q, :L] == want[k]).all(), (where, k, np.flatnonzero((got[k][q, :L] != want[k]))[:5])
    assert (got["ep_steps"][q] == want["ep_steps"]).all() and (got["ep_success"][q] == want["ep_success"]).all(), (where, got["ep_steps"][q], want["ep_steps"])
    assert same_bits(got["ep_reward"][q], want["ep_reward"]), where
    assert untouched(got, q, L), (where, "records beyond length were written")


def same_logs(a, b):
    return all(same_bits(a[k].astype(np.float64), b[k].astype(np.float64)) for k in a)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------
def test_the_reference_episodes_are_the_known_ones():
    """By the oracle alone: the episode lengths the cases below rely on."""
    mc = oracle_logs("mountaincar", 3)
    assert mc[2]["ep_steps"].tolist() == [409, 1000, 108] and mc[2]["ep_success"].tolist() == [1, 0, 1]
    assert mc[3]["ep_steps"].tolist() == [115, 39, 44] and len(mc[3]["action"]) == 201
    ac = np.concatenate([l["ep_steps"] for l in oracle_logs("acrobot", 3)])
    assert ac.min() >= 48 and ac.max() <= 117 and all(l["ep_success"].all() for l in oracle_logs("acrobot", 3))
    assert all((l["ep_steps"] == 1000).all() for l in oracle_logs("cartpole", 3))
    for env in ("mountaincar", "acrobot", "cartpole"):              # the step loop is Frirl.episode_eval()
        rows = oracle_rows(env, 3)
        logs = oracle_logs(env, 3)
        assert (np.concatenate([l["ep_steps"] for l in logs]) == rows[1]).all() and (np.concatenate([l["ep_success"] for l in logs]) == rows[3]).all()
        assert same_bits(np.concatenate([l["ep_reward"] for l in logs]), rows[2])


@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_logs_equal_the_oracles(env):
    K = 3
    want = oracle_logs(env, K)
    T = K * (frirl_amd.demo_describe(env)["max_steps"] + 1)
    got = record(env, 1, K, T, starts_for(env, K), agent=agent_for(env))
    print("length", got["length"], "ep_steps", got["ep_steps"].tolist())
    for e, w in enumerate(want):
        assert_log_equals(got, e, w, (env, e))


# ---- 2. lane shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "cartpole"])
def test_lane_shapes_agree_bit_for_bit(env, hip_option):
    K = 3
    ms = frirl_amd.demo_describe(env)["max_steps"]
    starts = starts_for(env, K)
    E = len(case(env))
    first = record(env, 1, K, K * (ms + 1), starts)                 # automatic: a full wave per log
    for e, w in enumerate(oracle_logs(env, K)):
        assert (first["ep_steps"][e] == w["ep_steps"]).all()
    for H in (1, 4, 8):
        hip_option("rollout_record_slices", H)
        assert same_logs(record(env, 1, K, K * (ms + 1), starts), first), H
    for H in (0, 1, 4, 8):                                          # the same episodes as n = 3 logs of one episode each
        hip_option("rollout_record_slices", H)
        rows = record(env, K, 1, ms + 1, starts)
        for e in range(E):
            pos = 0
            for k in range(K):
                q, L = e * K + k, int(first["ep_steps"][e, k]) + 1
                assert int(rows["length"][q]) == L and int(rows["ep_steps"][q, 0]) == L - 1, (H, q)
                for name in ARRAYS:
                    assert same_bits(rows[name][q, :L].astype(np.float64), first[name][e, pos:pos + L].astype(np.float64)), (H, q, name)
                assert same_bits(rows["ep_reward"][q], first["ep_reward"][e, k:k + 1]) and rows["ep_success"][q, 0] == first["ep_success"][e, k]
                assert untouched(rows, q, L)
                pos += L
            assert pos == int(first["length"][e])


# ---- 3. K = 1 against frirl_hip_rollout_batch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("env,epsilon", [("mountaincar", 0.0), ("acrobot", 0.0), ("cartpole", 0.0), ("mountaincar", EPS), ("cartpole", EPS)])
def test_single_episodes_equal_the_batched_rollout_rows(env, epsilon, hip_option):
    import torch
    n = 3
    hip_option("rollout_batch_resident", 0)
    greedy = oracle_rows(env, n)
    if epsilon > 0:
        explore = oracle_rows(env, n, 0, epsilon)
        assert (greedy[1] != explore[1]).any(), "by the reference alone: exploration changes at least one row"
        if env == "cartpole":
            assert explore[1].min() >= 316 and explore[1].max() <= 946
    d = frirl_amd.demo_describe(env)
    agent = frirl_amd.demo_agent(d, DEV, epsilon=epsilon, no_random=0, seed=SEED, env_id_base=BASE) if epsilon > 0 else agent_for(env)
    prob = upload(case(env))[0]
    starts = starts_for(env, n)
    steps, reward, success, final = (x.cpu().numpy() for x in prob.rollout_batch(agent, n, start_states=tens(starts)))
    torch.cuda.synchronize()
    want = explore if epsilon > 0 else greedy
    assert (steps == want[1]).all() and (success == want[3]).all()
    got = record(env, n, 1, d["max_steps"] + 1, starts, agent=agent, prob=prob)
    assert (got["ep_steps"][:, 0] == steps).all() and (got["ep_success"][:, 0] == success).all() and (got["length"] == steps + 1).all()
    assert same_bits(got["ep_reward"][:, 0], reward)
    last = np.stack([got["obs"][q, steps[q]] for q in range(len(steps))])
    assert same_bits(last, final), "the last observation is not the state the batched roll-out ends on"


# ---- 4. exploration across episodes ----------------------------------------------------------------------------------------------
def test_exploration_keys_follow_the_episode():
    env, K = "mountaincar", 3
    want = oracle_logs(env, K, EPS)
    d = frirl_amd.demo_describe(env)
    agents, av, starts = case(env), d["grids"][-1], starts_for(env, K)
    differs = 0
    for e, a in enumerate(agents):                                   # by the oracle alone: episode 1 under key episode 0 is another episode
        a.restore(a.rant, a.rconc)
        ep = oracle_episode(a, av, starts[e * K + 1], d["max_steps"], EPS, BASE + e, 0)
        first = int(want[e]["ep_steps"][0]) + 1
        mine = want[e]["action"][first:first + int(want[e]["ep_steps"][1]) + 1]
        differs += int(len(ep) != len(mine) or [r[2] for r in ep] != mine.tolist())
    assert differs > 0
    assert any((w["ep_steps"] != g["ep_steps"]).any() for w, g in zip(want, oracle_logs(env, K))), "exploration was meant to change episodes"
    agent = frirl_amd.demo_agent(d, DEV, epsilon=EPS, no_random=0, seed=SEED, env_id_base=BASE)
    got = record(env, 1, K, K * (d["max_steps"] + 1), starts, agent=agent)
    for e, w in enumerate(want):
        assert_log_equals(got, e, w, (env, e, "exploring"))


# ---- 5. capacity and logs that are not recorded ------------------------------------------------------------------------------------
def test_capacity_cuts_and_refuses_episodes():
    env, K = "mountaincar", 3
    want = oracle_logs(env, K)[3]
    assert want["ep_steps"].tolist() == [115, 39, 44]
    starts = starts_for(env, K)
    only3 = tens(np.array([0, 0, 0, 1, 0, 0], np.uint8))            # the neighbours' logs stay sentinel: a write at index >= T would show there
    for T, length, ep_steps in ((150, 150, [115, 33, -1]), (117, 116, [115, -1, -1]), (116, 116, [115, -1, -1]), (2, 2, [1, -1, -1])):
        got = record(env, 1, K, T, starts, active=only3)
        assert int(got["length"][3]) == length and got["ep_steps"][3].tolist() == ep_steps, (T, got["length"][3], got["ep_steps"][3])
        for k in ("obs", "q_obs", "reward"):
            assert same_bits(got[k][3, :length], want[k][:length]), (T, k)
        for k in ("action", "success", "start"):
            assert (got[k][3, :length] == want[k][:length]).all(), (T, k)
        assert untouched(got, 3, length)
        pos = 0
        for k, s in enumerate(ep_steps):                            # per episode: the sum of the recorded step rewards in step order
            total = 0.0
            for r in (want["reward"][pos + 1:pos + 1 + s] if s > 0 else []):
                total = total + float(r)
            assert same_bits(got["ep_reward"][3, k:k + 1], np.array([total])), (T, k)
            assert int(got["ep_success"][3, k]) == (int(want["success"][pos + s]) if s >= 0 else 0), (T, k)
            pos += s + 1 if s >= 0 else 0
        assert got["ep_success"][3].tolist() == [1 if s == 115 else 0 for s in ep_steps]
        for e in (0, 1, 2, 4, 5):
            assert int(got["length"][e]) == 0 and (got["ep_steps"][e] == -1).all() and untouched(got, e), (T, e)


def test_logs_that_are_not_recorded():
    env, n, K = "mountaincar", 3, 1
    d = frirl_amd.demo_describe(env)
    T = d["max_steps"] + 1
    starts = starts_for(env, n)
    full = record(env, n, K, T, starts)
    prob = upload(case(env))[0]
    prob.nrules[4] = 0
    counts, active = [3, 0, 2, 3, 3, 7], [1, 1, 1, 0, 1, 1]           # 7: clamped to n
    rows_e = [3, 0, 2, 0, 0, 3]
    got = record(env, n, K, T, starts, prob=prob, row_count=tens(np.array(counts, np.int32)), active=tens(np.array(active, np.uint8)))
    for q in range(6 * n):
        e, j = divmod(q, n)
        if j < rows_e[e]:
            assert all(same_bits(got[k][q].astype(np.float64), full[k][q].astype(np.float64)) for k in got), q
            assert int(got["length"][q]) > 1
        else:
            assert int(got["length"][q]) == 0 and int(got["ep_steps"][q, 0]) == -1 and got["ep_reward"][q, 0] == 0 and got["ep_success"][q, 0] == 0, q
            assert untouched(got, q), q
    # start_states = NULL: every episode of every log of an agent is its values_def episode
    agent = agent_for(env, case(env)[3].start)
    got = record(env, 2, 2, 2 * T, None, agent=agent)
    w = oracle_logs(env, 3)[3]
    assert (got["ep_steps"][6:8] == 115).all() and int(got["length"][6]) == 232
    assert same_bits(got["obs"][6, :116], w["obs"][:116]) and same_bits(got["obs"][7, 116:232], w["obs"][:116])


def test_max_steps_zero_records_one_start_record_per_episode():
    """max_steps = 0: oracle_episode's step loop, range(1, max_steps + 1), is empty -- an episode is its start record, which carries
    the greedy pick at the un-quantised start; the episode ends on the iteration that began it."""
    env, n, K, T = "mountaincar", 3, 2, 4
    agents = case(env)[:2]
    av = frirl_amd.demo_describe(env)["grids"][-1]
    starts = starts_for(env, n * K)[:2 * n * K]                      # log q = e * n + j, episode k: row q * K + k
    agent = agent_for(env)
    agent.desc.max_steps = 0
    got = record(env, n, K, T, starts, agent=agent, prob=upload(agents)[0])
    picks = set()
    for q in range(2 * n):
        a = agents[q // n]
        a.restore(a.rant, a.rconc)
        recs = [oracle_episode(a, av, starts[q * K + k], 0) for k in range(K)]
        assert all(len(ep) == 1 for ep in recs)
        recs = [ep[0] for ep in recs]
        want = dict(obs=np.array([r[0] for r in recs]), q_obs=np.array([r[1] for r in recs]), action=np.array([r[2] for r in recs], np.int32),
                    reward=np.array([r[3] for r in recs]), success=np.array([r[4] for r in recs], np.int32), start=np.array([r[5] for r in recs], np.uint8),
                    ep_steps=np.zeros(K, np.int32), ep_reward=np.zeros(K), ep_success=np.zeros(K, np.int32))
        assert want["start"].tolist() == [1] * K and same_bits(want["obs"], starts[q * K:(q + 1) * K])
        assert_log_equals(got, q, want, (env, q, "max_steps = 0"))
        picks |= set(want["action"].tolist())
    print("picks", sorted(picks))


# ---- 6. record -> learn on the device ----------------------------------------------------------------------------------------------
def taught_reference(E, passes, skip=()):
    """TaughtMirror.replay of the oracle-built log of mountaincar agent 3 by E fresh students: (description, mirrors, consumed)."""
    d = frirl_amd.demo_describe("mountaincar")
    w = oracle_logs("mountaincar", 3)[3]
    log = {k: w[k][None] for k in ("obs", "q_obs", "action", "reward", "success", "start")}
    log["length"] = np.array([0 if e in skip else len(w["action"]) for e in range(E)], np.int32)
    mirrors = tr.mirrors_for(d, log, 512)
    return d, mirrors, [m.replay(log, e, passes=passes) for e, m in enumerate(mirrors)]


def test_record_then_learn_without_a_host_copy():
    import torch
    env, K, E = "mountaincar", 3, 8
    d, mirrors, consumed = taught_reference(E, 2)
    teacher = upload(case(env))[0]
    log = teacher.rollout_record(agent_for(env), 1, K, K * (d["max_steps"] + 1), start_states=tens(starts_for(env, K).reshape(6, K, 2)))
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 512, DEV)
    demo = log.demonstration(log=3, E=E)
    assert demo.obs.data_ptr() == log.obs[3].data_ptr() and demo.action.data_ptr() == log.action[3].data_ptr() and demo.desc.agent_stride == 0
    replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, demo, passes=2)
    torch.cuda.synchronize()
    assert int(log.length[3]) == 201 and consumed == [402] * E
    assert replayed.cpu().tolist() == consumed and refused.cpu().tolist() == [m.refused for m in mirrors]
    assert_matches_mirrors(d, prob, envs, mirrors, "record -> learn")
    assert mirrors[0].five.R > 2 ** 3, "the students were meant to learn rules"
    # one log per agent: the teachers learn their own logs from the same memory (n == 1)
    own = log.demonstration()
    assert own.L == 6 and own.desc.agent_stride == log.T and own.length.data_ptr() == log.length.data_ptr()


# ---- 7. the batch object -----------------------------------------------------------------------------------------------------------
def make_batch(env, E, maxR, keep):
    """frirl_hip_batch_create for a demo, as tests/test_hip_rollout_batch.py: test_batch_evaluate_scores_and_best builds it."""
    d = frirl_amd.demo_describe(env)
    nant = d["nant"]
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
    keep += [grid, rant0, rconc0, u, ve, ave]
    desc = BatchDesc()
    desc.nant, desc.U, desc.E, desc.maxR, desc.u, desc.ve = nant, d["U"], E, maxR, u.ctypes.data, ve.ctypes.data
    desc.R0, desc.rant0, desc.rconc0 = ncorner, rant0.ctypes.data, rconc0.ctypes.data
    ag = desc.agent
    ag.alpha, ag.gamma, ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"]
    ag.weight_significant, ag.skip_rules, ag.A, ag.env_kind, ag.max_steps, ag.no_random = d["weight_thr"], d["skip_rules"], d["A"], d["kind"], d["max_steps"], 1
    ag.reward_good_above, ag.qdiff_final_tolerance = d["reward_good_above"], d["qdiff_final_tolerance"]
    for k in range(nant):
        ag.grid_len[k], ag.grid_div[k], ag.values_def[k] = len(d["grids"][k]), d["grid_div"][k], d["values_def"][k]
    ag.grid_values, ag.action_ve = grid.ctypes.data, ave.ctypes.data
    b = frirl_amd.lib().frirl_hip_batch_create(C.byref(desc))
    assert b, frirl_amd.lib().frirl_hip_last_error()
    return b


def rulebase_of(b, e, nant, maxR):
    L = frirl_amd.lib()
    R = C.c_int32()
    rant, rconc = np.zeros((maxR, nant)), np.zeros(maxR)
    DP = C.POINTER(C.c_double)
    frirl_amd.check(L.frirl_hip_batch_get_rulebase(b, e, C.byref(R), rant.ctypes.data_as(DP), rconc.ctypes.data_as(DP)), "frirl_hip_batch_get_rulebase")
    return R.value, rant[: R.value].copy(), rconc[: R.value].copy()


def test_batch_teach(tmp_path):
    """frirl_hip_batch_teach on six loaded mountain-car rule bases: its argument errors (all but "a teacher whose nrules lies outside
    1..maxR", which no call of the batch API can produce), the untouched teacher, the students against the manual chain record ->
    demonstration -> learn on the same data, the result fields, a student mask, and training afterwards."""
    import torch
    env, K, passes, teacher = "mountaincar", 3, 2, 3
    agents = case(env)
    E, nant, maxR = len(agents), 3, 512
    path = tmp_path / "six.frirlrb.bin"
    with open(path, "wb") as f:
        for a in agents:
            f.write(np.int32(a.R0).tobytes())
            f.write(np.ascontiguousarray(np.concatenate([a.rant, a.rconc[:, None]], axis=1)).tobytes())
    L = frirl_amd.lib()
    keep = []
    b = make_batch(env, E, maxR, keep)
    try:
        nrec = C.c_int32()
        frirl_amd.check(L.frirl_hip_batch_load_rulebases(b, str(path).encode(), C.byref(nrec)), "frirl_hip_batch_load_rulebases")
        res = frirl_amd.TeachResult()
        for bad in (dict(teacher=-1), dict(teacher=E), dict(episodes=0), dict(episodes=-2), dict(passes=0), dict(passes=1025), dict(episodes=2 ** 31 - 1)):
            kw = dict(dict(teacher=teacher, episodes=K, passes=passes), **bad)
            assert L.frirl_hip_batch_teach(b, kw["teacher"], kw["episodes"], None, kw["passes"], None, C.byref(res)) == -2, bad
            assert b"frirl_hip_batch_teach" in L.frirl_hip_last_error()
        before = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        assert [r[0] for r in before] == [a.R0 for a in agents]
        starts = np.ascontiguousarray(starts_for(env, K)[teacher * K:(teacher + 1) * K])
        res = frirl_amd.batch_teach(b, teacher, K, start_states=starts, passes=passes)
        after = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        # the teacher: untouched bit for bit
        assert after[teacher][0] == before[teacher][0] and same_bits(after[teacher][1], before[teacher][1]) and same_bits(after[teacher][2], before[teacher][2])
        # the students: the manual chain record -> demonstration -> learn on the same data
        prob, rant, _ = upload(agents, with_uidx=True, maxR=maxR)
        agent = agent_for(env)
        envs = frirl_amd.Envs(prob, DEV, rant_init=rant)
        log = prob.rollout_record(agent, 1, K, K * (agent.desc.max_steps + 1), start_states=tens(starts_for(env, K).reshape(E, K, 2)))
        demo = log.demonstration(log=teacher, E=E)
        demo.length[teacher] = 0
        replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, demo, passes=passes)
        torch.cuda.synchronize()
        nr, rb, ra = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), envs.rant.cpu().numpy()
        changed = 0
        for e in range(E):
            R = int(nr[e])
            assert after[e][0] == R, e
            assert (after[e][1] == ra[e, :, :R].T).all(), e
            assert within_contract(after[e][2], rb[e, nant, :R]).all(), e
            changed += int(R != before[e][0] or not same_bits(after[e][2], before[e][2]))
        assert changed == E - 1, "every student was meant to learn something, the teacher nothing"
        w = oracle_logs(env, K)[teacher]
        assert (res.teacher, res.episodes_recorded, res.successes, res.records) == (teacher, K, int(w["ep_success"].sum()), len(w["action"]))
        assert (res.students, res.refused, res.records_replayed) == (E - 1, int(refused.sum()), int(replayed.sum()))
        assert res.records == 201 and res.records_replayed == (E - 1) * passes * 201 and int(replayed[teacher]) == 0
        # a student mask, NULL start states (values_def: this batch has no desc.start_states), one pass
        mask = np.array([1, 0, 0, 1, 0, 1], np.uint8)               # the teacher's own flag is ignored
        res = frirl_amd.batch_teach(b, teacher, 2, passes=1, students=mask)
        assert (res.students, res.episodes_recorded) == (2, 2) and res.records_replayed == 2 * res.records
        again = [rulebase_of(b, e, nant, maxR) for e in range(E)]
        for e in (1, 2, 3, 4):
            assert again[e][0] == after[e][0] and same_bits(again[e][2], after[e][2]), e
        eps = C.c_int32(-1)
        assert L.frirl_hip_batch_train(b, 3, C.byref(eps)) == 0, L.frirl_hip_last_error()
        assert eps.value >= 0
    finally:
        L.frirl_hip_batch_destroy(b)


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------
def test_demo_teach_best(tmp_path):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    base = [demo, "--env", "mountaincar", "--agents", "8", "--evaluate", "2"]
    plain = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path)
    taught = subprocess.run(base + ["--teach-best", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert plain.returncode == 0 and taught.returncode == 0, (plain.stderr, taught.stderr)
    lines = taught.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("taught:")]
    assert len(at) == 1, taught.stdout
    assert "\n".join(lines[: at[0]]) + "\n" == plain.stdout, "without the new flags the output is what it was"
    fields = lines[at[0]].split()
    got = dict(zip(fields[1::2], fields[2::2]))
    assert list(got) == ["teacher", "episodes_recorded", "successes", "records", "students", "refused", "records_replayed"]
    assert got["students"] == "7" and int(got["episodes_recorded"]) == 2 and int(got["records_replayed"]) == 7 * int(got["records"])
    rest = lines[at[0] + 1:]
    assert len(rest) == len(plain.stdout.splitlines()) and all(l.startswith("evaluate mountaincar:") for l in rest), taught.stdout
