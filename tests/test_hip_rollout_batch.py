"""Greedy roll-outs on EVERY agent's own rule base in one call (frirl_hip_rollout_batch, csrc/rollout_batch.hip) and the agents'
scores: against the oracle's episode_eval row by row, between the two kernel forms and every lane-group size, against the
caller-stepped path (frirl_hip_policy_batch_* driven by frirl_hip_env_step) with exploration, for rows that do not exist, step caps,
scores, and a Shepard power other than nant.  The rule bases are those of tests/test_hip_reduce_batch.py (trained by the oracle).

Comparisons of steps, success and final states are exact; reward against the oracle within 1e-9 * max(1, |reward|) (the bound of
tests/test_hip_shared.py), between device paths bit for bit (a sum of environment rewards in step order).  Exact comparisons leave no
room for an arg-max pick that two summation orders resolve differently; observed on an MI355X: none in any case of this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import frirl_amd
from tests.test_hip_reduce_batch import BatchDesc, agent_for, case, spread_starts, upload

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPREAD = {"mountaincar": 0.15, "acrobot": 0.05, "cartpole": 0.02}       # the spreads the rule bases were trained with
SENT = -7
SEED, BASE = 2024, 1000          # exploration stream of case 3; the oracle alone shows that this seed changes rows (asserted there)


def starts_for(env, n, seed0=40):
    """[E * n][nstates]: row 0 of agent e = its training start, rows 1 .. n-1 = spread_starts with seed seed0 + e"""
    agents = case(env)
    out = []
    for e, a in enumerate(agents):
        s = spread_starts(a.fr, n, SPREAD[env], seed=seed0 + e)
        s[0] = a.start
        out.append(s)
    return np.ascontiguousarray(np.concatenate(out))


@functools.lru_cache(maxsize=None)
def oracle_rows(env, n, p=0, epsilon=0.0):
    """Frirl.episode_eval() from every row's start on its agent's rule base: (starts, steps, reward, success, final).  Computed once."""
    agents = case(env)
    s = starts_for(env, n)
    Q = len(agents) * n
    steps, reward, success = np.zeros(Q, np.int32), np.zeros(Q), np.zeros(Q, np.int32)
    final = np.zeros((Q, s.shape[1]))
    for e, a in enumerate(agents):
        a.restore(a.rant, a.rconc)                                    # a reduction test may have run on this oracle before
        old_p = a.fr.five.c.p
        if p:
            a.fr.set_power(p)
        for j in range(n):
            q = e * n + j
            a.fr.set_start_state(s[q])
            a.fr.set_exploration(epsilon, 0 if epsilon > 0 else 1, SEED, BASE + q)
            a.fr.episode_eval()
            steps[q], reward[q], success[q], final[q] = a.fr.ep_steps, a.fr.ep_reward, a.fr.success, a.fr.last_states
        a.fr.set_exploration(0.0, 1, 0, 0)
        a.fr.set_start_state(a.start)
        a.fr.five.c.p = old_p
    return s, steps, reward, success, final


def tens(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(env, n, agent=None, prob=None, starts="own", **kw):
    """One call on the uploaded case; returns host arrays (steps, reward, success, final[, scores])."""
    import torch
    prob = prob or upload(case(env))[0]
    agent = agent or agent_for(env)
    s = tens(starts_for(env, n)) if isinstance(starts, str) else (None if starts is None else tens(starts))
    out = prob.rollout_batch(agent, n, start_states=s, **kw)
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in out[:4]]
    if kw.get("scores"):
        res.append(frirl_amd.rollout_scores(out[4]))
    return res


def assert_follows_oracle(got, want, sel=None):
    steps, reward, success, final = got[:4]
    _, wsteps, wreward, wsuccess, _ = want
    sel = np.ones(len(wsteps), bool) if sel is None else sel
    print("steps", steps[sel], wsteps[sel], "reward", reward[sel], wreward[sel])
    assert (steps[sel] == wsteps[sel]).all(), np.flatnonzero(sel & (steps != wsteps))
    assert (success[sel] == wsuccess[sel]).all()
    assert (np.abs(reward[sel] - wreward[sel]) <= 1e-9 * np.maximum(1.0, np.abs(wreward[sel]))).all()


def stepped(env, n, agent, starts, step_cap=None):
    """The caller-stepped path on the same rows: policy_batch_begin / _observe with frirl_hip_env_step as the environment (cartpole's
    own quantiser through q_obs, as tests/test_hip_policy_batch.py: demo_step_fn)."""
    import torch
    prob = upload(case(env))[0]
    rows = frirl_amd.PolicyBatchRows(prob.E, n, DEV, step_cap=step_cap)
    states = tens(starts)
    out = prob.policy_batch_begin(agent, rows, states)
    action = out[0]
    for t in range(agent.desc.max_steps):
        live = rows.done == 0
        obs, reward, success, q = frirl_amd.env_step(agent, torch.where(live, action, torch.zeros_like(action)), states)
        prob.policy_batch_observe(agent, rows, obs, reward, success, q_obs=q if env == "cartpole" else None, out=out)
        states = torch.where(live[:, None], obs, states)
        if t % 25 == 24 and int((rows.done == 0).sum()) == 0:
            break
    torch.cuda.synchronize()
    assert bool((rows.done != 0).all())
    return rows.ep_steps.cpu().numpy(), rows.ep_reward.cpu().numpy(), rows.success.cpu().numpy(), states.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all()


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
def test_rows_follow_the_oracle_and_end_where_the_stepped_path_ends(env):
    n = 5
    want = oracle_rows(env, n)
    got = run(env, n)
    assert_follows_oracle(got, want)
    assert len(set(got[0].tolist())) > 1, "the rows were meant to differ"
    st = stepped(env, n, agent_for(env), want[0])
    assert (st[0] == got[0]).all() and (st[2] == got[2]).all() and same_bits(st[1], got[1])
    assert same_bits(st[3], got[3]), "final states differ from the states the stepped path ends on"


# ---- 2. forms and shapes agree --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "acrobot"])
def test_forms_and_lane_shapes_agree(env, hip_option):
    n = 70                       # more rows than one workgroup of the 8-slice tiled shape holds (8), the last workgroup ragged
    agents = case(env)
    cap = frirl_amd.lib().frirl_hip_rollout_resident_rules(5 if env == "acrobot" else 3, 3, 0, frirl_amd.ENV_KINDS[env])
    assert cap >= max(a.R0 for a in agents), "every agent fits the resident form"
    hip_option("rollout_batch_resident", 0)
    first = run(env, n)
    spot = oracle_rows(env, 5)                                        # the first rows of every agent are those of case 1
    for e in range(len(agents)):
        assert (first[0][e * n] == spot[1][e * 5]) and first[2][e * n] == spot[3][e * 5]
    runs = {"tiled": first}
    hip_option("rollout_batch_resident", 1)
    runs["resident"] = run(env, n)
    for H in (1, 4, 16, 64):
        hip_option("rollout_batch_slices", H)
        runs[f"H={H}"] = run(env, n)
    hip_option("rollout_batch_slices", 0)
    if env == "mountaincar":
        hip_option("rollout_batch_resident_rules", 120)
        assert sorted(a.R0 <= 120 for a in agents) == [False] * 3 + [True] * 3, "three agents to each form"
        runs["split"] = run(env, n)
    for name, r in runs.items():
        assert (r[0] == first[0]).all() and (r[2] == first[2]).all(), name
        assert same_bits(r[3], first[3]) and same_bits(r[1], first[1]), name
    assert (first[0] > 0).all() and len(set(first[0].tolist())) > 10


# ---- 3. against the stepped path, with exploration -------------------------------------------------------------------------------
def test_exploring_rows_equal_the_stepped_path():
    env, n = "mountaincar", 5
    greedy, explore = oracle_rows(env, n), oracle_rows(env, n, 0, 0.3)
    assert (greedy[1] != explore[1]).any(), "by the reference alone: exploration changes at least one row"
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV, epsilon=0.3, no_random=0, seed=SEED, env_id_base=BASE)
    got = run(env, n, agent=agent)
    assert_follows_oracle(got, explore)
    assert (got[0] != run(env, n)[0]).any()
    st = stepped(env, n, agent, explore[0])
    assert (st[0] == got[0]).all() and (st[2] == got[2]).all()
    assert same_bits(st[1], got[1]) and same_bits(st[3], got[3])


# ---- 4. rows that do not exist ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 1])
def test_rows_that_do_not_exist(resident, hip_option):
    import torch
    env, n = "mountaincar", 5
    hip_option("rollout_batch_resident", resident)
    want = oracle_rows(env, n)
    prob = upload(case(env))[0]
    E, Q, ns = prob.E, prob.E * n, prob.nant - 1
    counts = [5, 0, 3, 5, 5, 9]                                       # 9: clamped to n
    active = [1, 1, 1, 0, 1, 1]
    prob.nrules[4] = 0
    rows_e = np.array([min(c, n) if a and e != 4 else 0 for e, (c, a) in enumerate(zip(counts, active))])
    exists = (np.arange(Q) % n) < rows_e[np.arange(Q) // n]
    pad = 3                                                           # entries beyond E * n keep the sentinel too
    out = (torch.full((Q + pad,), SENT, dtype=torch.int32, device=DEV), torch.full((Q + pad,), float(SENT), dtype=torch.float64, device=DEV),
           torch.full((Q + pad,), SENT, dtype=torch.int32, device=DEV), torch.full((Q + pad, ns), float(SENT), dtype=torch.float64, device=DEV))
    views = tuple(o[:Q] for o in out)
    prob.rollout_batch(agent_for(env), n, start_states=tens(want[0]), row_count=tens(np.array(counts, np.int32)),
                       active=tens(np.array(active, np.uint8)), out=views)
    torch.cuda.synchronize()
    steps, reward, success, final = (o.cpu().numpy() for o in out)
    assert all((o[Q:] == SENT).all() for o in (steps, reward, success, final))
    gone = ~exists
    assert (steps[:Q][gone] == -1).all() and (reward[:Q][gone] == 0).all() and (success[:Q][gone] == 0).all() and (final[:Q][gone] == SENT).all()
    assert_follows_oracle((steps[:Q], reward[:Q], success[:Q], final[:Q]), want, exists)
    assert exists.sum() == 5 + 3 + 5 and (final[:Q][exists] != SENT).all()
    # start_states = NULL: every row of an agent is its values_def episode
    prob = upload(case(env))[0]
    agent = agent_for(env, case(env)[2].start)
    got = run(env, n, agent=agent, prob=prob, starts=None)
    for e in range(E):
        assert (got[0][e * n:(e + 1) * n] == got[0][e * n]).all() and same_bits(got[1][e * n:(e + 1) * n], np.full(n, got[1][e * n]))
    assert got[0][2 * n] == want[1][2 * n] and got[2][2 * n] == want[3][2 * n]          # agent 2 from its own training start


# ---- 5. step cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 1])
def test_step_cap_per_agent(resident, hip_option):
    env, n = "mountaincar", 5
    hip_option("rollout_batch_resident", resident)
    want = oracle_rows(env, n)
    free = run(env, n)
    E = len(case(env))
    assert want[1][1 * n:2 * n].min() > 7 and want[1][3 * n:4 * n].min() > 1, "known episodes longer than the caps"
    caps = np.array([100000, 7, 1000, 1, 0, 1000], np.int32)          # above max_steps = max_steps; 0 is clamped to 1
    got = run(env, n, step_cap=tens(caps))
    eff = np.clip(caps, 1, 1000).repeat(n)
    assert (got[0] == np.minimum(free[0], eff)).all()
    cut = free[0] > eff
    assert cut[n:2 * n].all() and (got[2][cut] == 0).all() and (got[0][cut] == eff[cut]).all()
    keep = ~cut
    assert (got[2][keep] == free[2][keep]).all() and same_bits(got[1][keep], free[1][keep]) and same_bits(got[3][keep], free[3][keep])
    st = stepped(env, n, agent_for(env), want[0], step_cap=tens(np.clip(caps, 1, 1000).astype(np.int32)))
    assert (st[0] == got[0]).all() and same_bits(st[1], got[1]) and same_bits(st[3], got[3])
    assert E == 6


# ---- 6. scores --------------------------------------------------------------------------------------------------------------------
def host_scores(steps, reward, success, E, n):
    out = []
    for e in range(E):
        rows = succ = ssum = 0
        rsum = rmin = rmax = 0.0
        for j in range(n):
            q = e * n + j
            if steps[q] < 0:
                continue
            r = float(reward[q])
            rmin = r if rows == 0 or r < rmin else rmin
            rmax = r if rows == 0 or r > rmax else rmax
            rows += 1
            succ += int(success[q] == 1)
            ssum += int(steps[q])
            rsum = rsum + r
        out.append((rows, succ, ssum, rsum, rmin, rmax))
    return out


def score_tuple(s):
    return (s.rows, s.successes, s.steps_sum, s.reward_sum, s.reward_min, s.reward_max)


def best_of(scores):
    return max(range(len(scores)), key=lambda e: (scores[e][1], scores[e][3], -e))


@pytest.mark.parametrize("resident", [0, 1])
def test_scores_equal_a_host_loop_in_row_order(resident, hip_option):
    env, n = "acrobot", 5
    hip_option("rollout_batch_resident", resident)
    counts = np.array([5, 5, 0, 2], np.int32)
    steps, reward, success, final, sc = run(env, n, row_count=tens(counts), scores=True)
    want = host_scores(steps, reward, success, 4, n)
    for e in range(4):
        got = score_tuple(sc[e])
        assert got[:3] == want[e][:3] and same_bits(np.array(got[3:]), np.array(want[e][3:])), (e, got, want[e])
    assert sc[2].rows == 0 and score_tuple(sc[2]) == (0, 0, 0, 0.0, 0.0, 0.0) and sc[3].rows == 2
    assert_follows_oracle((steps, reward, success, final), oracle_rows(env, n), steps >= 0)


def test_batch_evaluate_scores_and_best(tmp_path):
    """frirl_hip_batch_evaluate on a library-owned batch that loaded the same six rule bases: the scores of frirl_hip_rollout_batch and
    the best agent by the host rule."""
    env, n = "mountaincar", 5
    agents = case(env)
    E = len(agents)
    path = tmp_path / "six.frirlrb.bin"
    with open(path, "wb") as f:                                       # E records of frirl_save_rb_to_bin_file
        for a in agents:
            f.write(np.int32(a.R0).tobytes())
            f.write(np.ascontiguousarray(np.concatenate([a.rant, a.rconc[:, None]], axis=1)).tobytes())
    L = frirl_amd.lib()
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
    desc = BatchDesc()
    desc.nant, desc.U, desc.E, desc.maxR, desc.u, desc.ve = nant, d["U"], E, 512, u.ctypes.data, ve.ctypes.data
    desc.R0, desc.rant0, desc.rconc0 = ncorner, rant0.ctypes.data, rconc0.ctypes.data
    ag = desc.agent
    ag.alpha, ag.gamma, ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"]
    ag.weight_significant, ag.skip_rules, ag.A, ag.env_kind, ag.max_steps, ag.no_random = d["weight_thr"], d["skip_rules"], d["A"], d["kind"], d["max_steps"], 1
    ag.reward_good_above, ag.qdiff_final_tolerance = d["reward_good_above"], d["qdiff_final_tolerance"]
    for k in range(nant):
        ag.grid_len[k], ag.grid_div[k], ag.values_def[k] = len(d["grids"][k]), d["grid_div"][k], d["values_def"][k]
    ag.grid_values, ag.action_ve = grid.ctypes.data, ave.ctypes.data
    starts = starts_for(env, n)
    steps, reward, success, final, sc = run(env, n, scores=True)
    want = [score_tuple(s) for s in sc]
    assert want == [tuple(w) for w in host_scores(steps, reward, success, E, n)]
    b = L.frirl_hip_batch_create(C.byref(desc))
    assert b, L.frirl_hip_last_error()
    try:
        nrec = C.c_int32()
        frirl_amd.check(L.frirl_hip_batch_load_rulebases(b, str(path).encode(), C.byref(nrec)), "frirl_hip_batch_load_rulebases")
        assert nrec.value == E
        got = (frirl_amd.RolloutScore * E)()
        best = C.c_int32(-1)
        frirl_amd.check(L.frirl_hip_batch_evaluate(b, n, starts.ctypes.data_as(C.POINTER(C.c_double)), got, C.byref(best)), "frirl_hip_batch_evaluate")
        assert [score_tuple(s) for s in got] == want
        assert best.value == best_of(want)
        assert len({w[3] for w in want}) > 1, "the agents were meant to score differently"
        # NULL start states: every row at the agent's own start (values_def: this batch has no desc.start_states)
        frirl_amd.check(L.frirl_hip_batch_evaluate(b, 3, None, got, C.byref(best)), "frirl_hip_batch_evaluate")
        assert all(s.rows == 3 and s.reward_min == s.reward_max for s in got)
    finally:
        L.frirl_hip_batch_destroy(b)


# ---- 7. a Shepard power other than nant -------------------------------------------------------------------------------------------
def test_shepard_power_two_runs_the_tiled_form(hip_option):
    env, n = "acrobot", 3
    want = oracle_rows(env, n, 2)
    assert (want[1] != oracle_rows(env, n)[1]).any(), "by the reference alone: the power changes at least one episode"
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV, p=2)
    assert frirl_amd.lib().frirl_hip_rollout_resident_rules(5, 3, 2, frirl_amd.ENV_KINDS[env]) == 0
    got = run(env, n, agent=agent)
    assert_follows_oracle(got, want)
    for opt, v in (("rollout_batch_resident", 1), ("rollout_batch_slices", 16), ("rollout_batch_resident_rules", 400)):
        hip_option(opt, v)
        again = run(env, n, agent=agent)
        assert all(same_bits(a.astype(np.float64), g.astype(np.float64)) for a, g in zip(again, got)), opt


# ---- 8. no step allowed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 1])
def test_max_steps_zero_ends_every_row_on_its_start(resident, hip_option):
    """max_steps = 0: the reference's step loop, range(1, max_steps + 1), is empty.  The tiled form never enters its loop, the resident
    form ends the row on the iteration of its start sweep."""
    env, n = "mountaincar", 3
    hip_option("rollout_batch_resident", resident)
    # which form serves the two agents: 0 = never the resident one; 1 = wherever it fits, and by the library's own capacity both fit
    cap = frirl_amd.lib().frirl_hip_rollout_resident_rules(3, 3, 0, frirl_amd.ENV_KINDS[env])
    assert cap >= max(a.R0 for a in case(env)[:2]), "both agents fit the resident form"
    starts = starts_for(env, n)[:2 * n]
    agent = agent_for(env)
    agent.desc.max_steps = 0
    steps, reward, success, final = run(env, n, agent=agent, prob=upload(case(env)[:2])[0], starts=starts)
    assert (steps == 0).all() and (reward == 0.0).all() and (success == 0).all() and len(steps) == 2 * n
    assert same_bits(final, starts), "no step: the final state is the start state"
