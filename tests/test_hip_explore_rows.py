"""Per-agent exploration rows (frirl_hip_explore_rows) on the device: a launch in which agent e picks at its own epsilon, annealed
linearly to zero over its own horizon, against the oracle's construct loop run one episode per call at that episode's rate.  The
cases and the conditions under which they tell a wrong row from the right one are in tests/explore_rows_cases.py, asserted on the CPU
by tests/test_explore_rows_ref.py.

1. the persistent learner (frirl_hip_learn_train_explore) per agent against its oracle chain, alone and with hyper-parameter rows
2. an epsilon column equal to the agent's epsilon, no horizon: byte-identical to frirl_hip_learn_train and _train_rows
3. caller-stepped agents (frirl_hip_agent_begin_explore / _observe_explore) against per-agent mirrors; no rows = the _rows call
4. the batch object (frirl_hip_batch_set_exploration) and frirl_demo --explore

Bars: decisions, counters, reward bits, appended antecedents exact; consequents <= 1e-9 relative (the contract is 1e-6).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests.test_hip_external import Mirror, PointEnv, point_desc

DEV = "cuda"
TOL = 1e-9
gpu = pytest.mark.gpu


def check_against_chain(r, e, prob, envs, run):
    """Agent e of a finished learner run against its oracle chain r (explore_rows_cases.chain)."""
    from tests.test_hip_learn import check_agent_against_oracle
    fr = r["fr"]
    got = (int(run.conv.converged[e]), int(run.conv.episodes[e]), int(run.steps_total[e]))
    assert got == (r["converged"], r["episodes"], r["total_steps"]), (e, got, (r["converged"], r["episodes"], r["total_steps"]))
    assert int(envs.ep_steps[e]) == fr.ep_steps and xc.bits(float(envs.ep_reward[e])) == xc.bits(fr.ep_reward), e
    assert int(envs.fus[e]) == int(fr.fus), e
    check_agent_against_oracle(fr, prob, envs, e)


# ---- 1. the persistent learner -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env,slices,budget", [(env, s, 700) for env in xc.DEMOS for s in (0, 1, 64)] + [("acrobot", 0, 5), ("cartpole", 0, 5)])
def test_persistent_learner_follows_each_agents_own_chain(env, slices, budget, hip_option):
    """The cases of explore_rows_cases.CASES (9 / 12 / 12 agents, ids 77 + e, agent e under set e mod nsets) through
    frirl_hip_learn_train_explore at the default lane-group size and at 1 and 64 rule slices with a budget of 700 steps, and on
    acrobot and cartpole at a budget of 5, where every launch boundary falls inside an episode (the queue re-sorts the agents between
    launches: a row taken by launch slot would be another agent's)."""
    import torch
    E, sets, seed, N = xc.CASES[env]
    dev0 = torch.device("cuda", 0)
    if slices:
        hip_option("learn_slices", slices)
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=seed, env_id_base=xc.ID_BASE)
    assert frirl_amd.learn_supported(prob, agent) and agent.desc.epsilon == 0.0
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns(xc.agent_sets(env)))
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=N, budget=budget, explore=explore)
    torch.cuda.synchronize()
    for e in range(E):
        check_against_chain(xc.agent_run(env, e), e, prob, envs, run)
    if budget == 5:
        assert run.launches > max(xc.agent_run(env, e)["total_steps"] for e in range(E)) // 24


@gpu
def test_exploration_rows_beside_hyper_parameter_rows():
    """Acrobot, 12 agents, 8 episodes, hyper-parameter set e mod 6 of the rows test's demo sets crossed with exploration set e mod 4
    (explore_rows_cases.cross_sets), both structs in one frirl_hip_learn_train_explore: every agent against the oracle chain with
    both applied."""
    import torch
    from tests import hparam_rows_cases as rc
    env, E = xc.CROSS_ENV, xc.CROSS_E
    seed, N = xc.CASES[env][2], xc.CROSS_EPISODES
    dev0 = torch.device("cuda", 0)
    pairs = xc.cross_sets()
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=seed, env_id_base=xc.ID_BASE)
    rows = frirl_amd.HparamRows(E, dev0, **rc.columns([hc.demo_desc(env, name) for name, _ in pairs]))
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns([x for _, x in pairs]))
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=N, budget=700, rows=rows, explore=explore)
    torch.cuda.synchronize()
    for e in range(E):
        check_against_chain(xc.cross_run(e), e, prob, envs, run)


# ---- 2. rows that repeat the agent's epsilon ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env", xc.DEMOS)
def test_an_epsilon_column_equal_to_the_agents_changes_nothing(env):
    """21 agents with start states spread over the state grids, agent.epsilon = 0.3, no_random = 0: frirl_hip_learn_train, then
    frirl_hip_learn_train_rows with all six columns, then frirl_hip_learn_train_explore with an epsilon column of 0.3 and no horizon,
    with a horizon column of zeros too, and with both structs NULL -- every state array byte for byte the same."""
    import torch
    from tests import hparam_rows_cases as rc
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    E = 21
    dev0 = torch.device("cuda", 0)
    d = hc.demo_desc(env, "default")
    rng = np.random.default_rng(17)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))).to(dev0)
    forms = [dict(),
             dict(rows=frirl_amd.HparamRows(E, dev0, **rc.columns([d] * E))),
             dict(explore=frirl_amd.ExploreRows(E, dev0, epsilon=np.full(E, 0.3))),
             dict(explore=frirl_amd.ExploreRows(E, dev0, epsilon=np.full(E, 0.3), horizon=np.zeros(E, dtype=np.int32))),
             dict(explore=frirl_amd.ExploreRows(E, dev0)),
             dict(explore=frirl_amd.ExploreRows.null(E))]
    outs = []
    for kw in forms:
        prob, agent, envs = frirl_amd.fresh_batch(d, E, hc.TRAJ_MAXR, dev0, start_states=start, epsilon=0.3, no_random=0, seed=1234, env_id_base=xc.ID_BASE)
        run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=hc.TRAJ_EPISODES[env], budget=700, **kw)
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the start states were meant to desynchronise the agents"
    for o, what in zip(outs[1:], ("hyper-parameter rows", "epsilon column", "epsilon and horizon columns", "all-NULL exploration struct", "both structs NULL")):
        assert_same(outs[0], o, what)


# ---- 3. caller-stepped agents ----------------------------------------------------------------------------------------------------------
class ExploreMirror(Mirror):
    """tests/test_hip_external.py::Mirror whose pick is tests/explore_ref.py's at the rate of the episode: epsilon `eps` falling to
    zero over `horizon` episodes (explore_rows_cases.epsilon_at)."""

    def __init__(self, d, start, maxR, eps, horizon, seed, gid):
        super().__init__(d, start, maxR, explore=dict(epsilon=eps, seed=seed), gid=gid)
        self.eps, self.horizon = eps, horizon

    def explore_episode(self, env, picks, key):
        """The episode whose stream key is `key` (frirl_hip_agent_begin: episode[e] + 1)."""
        assert key == self.episode_no + 1
        self.explore["epsilon"] = xc.epsilon_at(self.eps, self.horizon, key)
        return self.episode(env, picks)


def point_mirrors(nant, A):
    """Environment, start states and one mirror per agent of the caller-stepped case (no GPU needed)."""
    d = xc.point_description(nant, A)
    starts = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, (xc.POINT_E, nant - 1)))
    mirrors = [ExploreMirror(d, starts[e], xc.POINT_MAXR, eps, h, xc.POINT_SEED, xc.ID_BASE + e) for e, (eps, h) in enumerate(xc.point_pairs())]
    return PointEnv(nant - 1), starts, mirrors


@gpu
@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_caller_stepped_agents_follow_each_agents_own_rate(nant, A):
    """16 agents, 5 episodes of the torch point environment through frirl_hip_agent_begin_explore / _observe_explore, agent e with
    epsilon 0.4 over a horizon of e mod 4 episodes (one agent in four is never annealed; episodes cross every horizon), against a
    mirror that picks at the rate of the episode.  A pick may follow the device only inside Mirror.pick's 1e-12 tie of the oracle, at
    most 10 % of the shape's picks; consequents at 1e-9.  The 2 x 32 shape runs on a description whose action universe gives each
    of the 32 actions a point of its own (explore_rows_cases.point_description); A = 32 is where the clamp of round(u * A) acts."""
    import torch
    d = xc.point_description(nant, A)
    env, starts, mirrors = point_mirrors(nant, A)
    E, maxR = xc.POINT_E, xc.POINT_MAXR
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV, no_random=0, seed=xc.POINT_SEED, env_id_base=xc.ID_BASE)
    explore = frirl_amd.ExploreRows(E, DEV, **xc.columns(xc.point_pairs()))
    conv = frirl_amd.Convergence(prob, DEV)
    ss = torch.from_numpy(starts).to(DEV)
    for ep in range(xc.POINT_EPISODES):
        _, aidx = frirl_amd.agent_begin(prob, agent, envs, ss, explore=explore)
        envs.done.copy_(torch.maximum(envs.done, conv.converged))          # converged agents sit the episode out (frirl_amd.train)
        chosen = [aidx.clone()]
        live = [(envs.done == 0).clone()]
        action = agent.grid_values[nant - 1][aidx.long()]
        for t in range(d["max_steps"]):
            obs, reward, success = env.step(torch, envs.states, action)
            nxt, nidx = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32), explore=explore)
            chosen.append(nidx.clone())
            live.append((envs.done == 0).clone())
            action = torch.where(live[-2], nxt, action)
        conv.update(prob, agent, envs)
        torch.cuda.synchronize()
        was_live = [l.cpu().numpy() for l in live]
        picks = [c.cpu().numpy() for c in chosen]
        rant, rb, nrules = envs.rant.cpu().numpy(), prob.rb.cpu().numpy(), prob.nrules.cpu().numpy()
        for e, m in enumerate(mirrors):
            if m.converged:
                assert not was_live[0][e] and int(conv.converged[e]) == 1
                continue
            actions, steps, total = m.explore_episode(env, [int(p[e]) for p in picks], ep + 1)
            got = [int(picks[t][e]) for t in range(len(actions))]
            assert got == actions, (nant, A, ep, e)
            assert int(envs.ep_steps[e]) == steps and float(envs.ep_reward[e]) == total and int(envs.done[e]) == 1
            R = m.five.R
            assert int(nrules[e]) == R, (nant, A, ep, e)
            assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all()
            q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
            assert (np.abs(q - ref) <= TOL * np.maximum(np.abs(ref), 1e-9)).all(), (nant, A, ep, e)
            assert int(envs.fus[e]) == int(m.fus)
            assert int(conv.converged[e]) == int(m.converged), (nant, A, ep, e)
    ties, picks_made = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, "ties", ties, "picks", picks_made, "explored", [m.explored for m in mirrors], "clamped", sum(m.clamped for m in mirrors))
    assert ties * 10 <= picks_made, (ties, picks_made)
    assert all(m.explored > 0 for m in mirrors)


@gpu
def test_no_exploration_rows_are_the_rows_call():
    """frirl_hip_agent_begin_explore / _observe_explore with an all-NULL exploration struct and with a NULL one against
    frirl_hip_agent_begin_rows / _observe_rows on twin batches that explore at the agent's epsilon, 30 steps of the point
    environment: the same bytes after every call."""
    import torch
    from tests.test_hip_external import assert_same, state_arrays
    nant, A, E = 4, 5, 64
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    ss = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(9).uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    rows = frirl_amd.HparamRows(E, DEV)
    sides = [dict(rows=rows), dict(rows=rows, explore=frirl_amd.ExploreRows(E, DEV)), dict(explore=frirl_amd.ExploreRows.null(E))]
    batches = [frirl_amd.fresh_batch(d, E, 512, DEV, epsilon=0.25, no_random=0, seed=99, env_id_base=5) for _ in sides]
    acts = [frirl_amd.agent_begin(p, a, ev, ss, **kw)[0] for (p, a, ev), kw in zip(batches, sides)]
    for (p, a, ev) in batches[1:]:
        assert_same(state_arrays(batches[0][0], batches[0][2]), state_arrays(p, ev), "begin")
    for t in range(30):
        for i, ((p, a, ev), kw) in enumerate(zip(batches, sides)):
            o, r, s = env.step(torch, ev.states, acts[i])
            n, _ = frirl_amd.agent_observe(p, a, ev, o.contiguous(), r.contiguous(), s.to(torch.int32), **kw)
            acts[i] = torch.where(ev.done == 0, n, acts[i])
        for (p, a, ev) in batches[1:]:
            assert_same(state_arrays(batches[0][0], batches[0][2]), state_arrays(p, ev), t)
    assert int(batches[0][0].nrules.max()) > 2 ** nant


# ---- 4. batch object and demo --------------------------------------------------------------------------------------------------------
@gpu
def test_batch_object_trains_under_exploration_rows():
    """Nine mountaincar agents of a library-owned batch (seed 1265, ids 77 + e; the batch itself is greedy, no_random = 1) through
    frirl_hip_batch_set_exploration and frirl_hip_batch_train: frirl_hip_batch_agent_report gives every agent the verdict, episodes,
    rules and last episode of its chain.  While the rows are set the four calls that do not honour them refuse, naming themselves,
    and a rejected set leaves them in place; after clearing, frirl_hip_batch_episode runs again and training is greedy."""
    lib = frirl_amd.lib()
    env = "mountaincar"
    E, sets, seed, N = xc.CASES[env]
    col = xc.columns(xc.agent_sets(env))
    batch = frirl_amd.demo_batch_object(env, E, xc.MAXR, seed=seed, env_id_base=xc.ID_BASE)
    try:
        frirl_amd.batch_set_exploration(batch, **col)
        ran = C.c_int32(0)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, N, C.byref(ran)), "frirl_hip_batch_train")
        rep = frirl_amd.batch_agent_report(batch)
        for e in range(E):
            r = xc.agent_run(env, e)
            fr = r["fr"]
            got = (int(rep["converged"][e]), int(rep["episodes"][e]), int(rep["rules"][e]), int(rep["ep_steps"][e]), xc.bits(rep["ep_reward"][e]))
            assert got == (r["converged"], r["episodes"], fr.five.R, fr.ep_steps, xc.bits(fr.ep_reward)), (e, got)
        assert ran.value == N - 1
        st = frirl_amd.BatchStats()
        frirl_amd.check(lib.frirl_hip_batch_stats(batch, C.byref(st)), "frirl_hip_batch_stats")
        assert st.total_env_steps == xc.MEASURED[env]["total_steps"]
        assert lib.frirl_hip_batch_episode(batch) == -2 and b"frirl_hip_batch_episode" in lib.frirl_hip_last_error()
        res = frirl_amd.TeachResult()
        assert lib.frirl_hip_batch_teach(batch, 0, 1, None, 1, None, C.byref(res)) == -2 and b"frirl_hip_batch_teach" in lib.frirl_hip_last_error()
        assert lib.frirl_hip_batch_merge_round(batch, None) == -2 and b"frirl_hip_batch_merge_round" in lib.frirl_hip_last_error()
        er, rounds = C.c_int32(0), C.c_int32(0)
        assert lib.frirl_hip_batch_train_merged(batch, 4, 2, C.byref(er), C.byref(rounds)) == -2 and b"frirl_hip_batch_train_merged" in lib.frirl_hip_last_error()
        with pytest.raises(frirl_amd.FrirlHipError, match="agent 4.*epsilon"):
            frirl_amd.batch_set_exploration(batch, epsilon=[0.5] * 4 + [1.5] + [0.5] * 4)
        with pytest.raises(frirl_amd.FrirlHipError, match="agent 2.*horizon"):
            frirl_amd.batch_set_exploration(batch, horizon=[0, 1, -1] + [0] * 6)
        assert lib.frirl_hip_batch_episode(batch) == -2, "a rejected set of rows must leave the batch as it was"
        frirl_amd.batch_set_exploration(batch, clear=True)
        assert lib.frirl_hip_batch_episode(batch) == 0
        assert (frirl_amd.batch_agent_report(batch)["episodes"] == rep["episodes"] + 1 - rep["converged"]).all()
    finally:
        lib.frirl_hip_batch_destroy(batch)
    # a fresh batch trained after set + clear is the greedy agent (the batch's own no_random holds again)
    batch = frirl_amd.demo_batch_object(env, 3, xc.MAXR, seed=seed, env_id_base=xc.ID_BASE)
    try:
        frirl_amd.batch_set_exploration(batch, epsilon=[0.3] * 3)
        frirl_amd.batch_set_exploration(batch, clear=True)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, N, None), "frirl_hip_batch_train")
        rep = frirl_amd.batch_agent_report(batch)
        r = xc.agent_run(env, 0)            # set 0: epsilon 0
        assert [(int(rep["converged"][e]), int(rep["episodes"][e]), int(rep["rules"][e])) for e in range(3)] == [(r["converged"], r["episodes"], r["fr"].five.R)] * 3
    finally:
        lib.frirl_hip_batch_destroy(batch)


DEMO_ID_BASE = 0            # frirl_demo numbers its agents from 0 (frirl_hip_agent.env_id_base of its batches) unless --id-base is given


@gpu
def test_demo_sweeps_three_exploration_sets_in_one_run(tmp_path):
    """frirl_demo --env mountaincar --agents 9 --seed 1265 --max-episodes 40 --explore f.txt: three `line` lines whose counts and means
    are the oracle chains'.  The demo's own id base is 0, at which seed 1265 does not keep the margin of the greedy picks
    (tests/test_explore_rows_ref.py::test_the_demo_case_at_the_demos_ids: 1.9e-7), so the run is given --id-base 77, the ids of the
    admitted case."""
    env = "mountaincar"
    E, sets, seed, N = xc.CASES[env]
    f = tmp_path / "f.txt"
    f.write_text("# epsilon horizon\n" + "".join(f"{eps!r} {h}   # set {s}\n" for s, (eps, h) in enumerate(sets)))
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    r = subprocess.run([demo, "--env", env, "--agents", str(E), "--seed", str(seed), "--max-episodes", str(N), "--explore", str(f), "--id-base", str(xc.ID_BASE)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(f"explore {env}: line ")]
    assert len(lines) == 3, r.stdout
    for s, line in enumerate(lines):
        m = re.match(rf"explore {env}: line (\d+) agents (\d+) converged (\d+) mean-episodes ([\d.]+) max-episodes (\d+) mean-rules ([\d.]+) mean-reward (-?[\d.]+)$", line)
        assert m, line
        runs = [xc.agent_run(env, e) for e in range(s, E, len(sets))]
        assert (int(m[1]), int(m[2]), int(m[3]), int(m[5])) == (s, len(runs), sum(x["converged"] for x in runs), max(x["episodes"] for x in runs)), line
        assert abs(float(m[4]) - np.mean([x["episodes"] for x in runs])) <= 6e-4 and abs(float(m[6]) - np.mean([x["fr"].five.R for x in runs])) <= 6e-4, line
        reward = np.mean([x["fr"].ep_reward for x in runs])
        assert abs(float(m[7]) - reward) <= 1e-6 * max(1.0, abs(reward)), line
