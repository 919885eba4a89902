"""Per-agent expected SARSA (frirl_hip_expect_rows) on the device: a launch in which a flagged agent learns towards the expectation of the
A conclusions at s' under its own epsilon-greedy pick, against the construct loop restated from the oracle's pieces with the gamma-0
form of the update (tests/expect_ref.py).  The cases and the conditions under which they tell the expectation from SARSA and from Q are
asserted on the CPU by tests/test_expect_ref.py.

1. the persistent learner (frirl_hip_learn_train_expect) per agent against its chain: every lane-group size, launch boundaries inside
   episodes, crossed with hyper-parameter rows
2. equivalences: an all-zero column, expected_all 0 and a NULL struct are frirl_hip_learn_train_target; all-expected without exploration
   is frirl_hip_learn_train; a flagged agent's target byte is not consulted
3. caller-stepped agents (frirl_hip_agent_observe_expect) against per-agent mirrors, taught and untaught; all-zero = the _target call
4. the batch object (frirl_hip_batch_set_expected / _get_expected, clone with inherit_rows) and frirl_demo --expected-rows

Bars: decisions, counters, reward bits, appended antecedents exact; consequents <= 1e-9 relative (the bar of
tests/test_hip_target.py for the same comparison).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import expect_ref as er
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc
from tests import target_ref as tr
from tests.test_hip_target import check_against_chain, differs_from, _report_matches

DEV = "cuda"
TOL = 1e-9
gpu = pytest.mark.gpu


def learner_run(env, dev0, budget, expect=None, target=None, **kw):
    E = xc.CASES[env][0]
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=er.SEEDS[env], env_id_base=xc.ID_BASE)
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns(xc.agent_sets(env)))
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=tr.EPISODES[env] + 1, budget=budget, explore=explore, target=target, expect=expect, **kw)
    return prob, agent, envs, run


# ---- 1. the persistent learner -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env,slices", [(env, s) for env in er.DEMOS for s in (0, 1, 4, 64)])
def test_persistent_learner_follows_each_agents_chain_under_the_mixed_column(env, slices, hip_option):
    """The agents of explore_rows_cases.CASES under expect_ref.SEEDS over 8 / 9 / 7 episodes with expected[e] = (e // nsets) % 2 and no
    target struct through frirl_hip_learn_train_expect, at the default lane-group size and at 1, 4 and 64 rule slices (cartpole has no
    one-lane kernel: 2 there).  Every agent follows the chain of its own mode; every exploring expected agent ends neither where its
    SARSA chain ends nor where its Q chain ends -- without the feature it would end on the former."""
    import torch
    E, sets, _, _ = xc.CASES[env]
    dev0 = torch.device("cuda", 0)
    if slices:
        hip_option("learn_slices", slices)
    col = er.mixed_column(env)
    prob, agent, envs, run = learner_run(env, dev0, 700, frirl_amd.ExpectRows(E, dev0, expected=col))
    torch.cuda.synchronize()
    told_apart = 0
    for e in range(E):
        check_against_chain(er.agent_run(env, e, er.mode_of(col[e])), e, prob, envs, run)
        if col[e] and sets[e % len(sets)][0] > 0:
            assert differs_from(er.agent_run(env, e, er.SARSA), e, prob), (e, "an exploring expected agent ended on its SARSA chain")
            assert differs_from(er.agent_run(env, e, er.Q), e, prob), (e, "an exploring expected agent ended on its Q chain")
            told_apart += 1
    assert told_apart >= len(sets) - 1


@gpu
@pytest.mark.parametrize("env", ["acrobot", "cartpole"])
def test_launch_boundaries_inside_episodes_change_nothing(env):
    """The same run with a budget of 5 steps per launch -- every launch boundary falls inside an episode, and the queue re-sorts the
    agents between launches, so a flag taken by launch slot would be another agent's -- against one with a budget no agent exhausts:
    every state array byte for byte the same (the rule-visit counters, a profiling aid, apart)."""
    import torch
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    E = xc.CASES[env][0]
    dev0 = torch.device("cuda", 0)
    col = er.mixed_column(env)
    outs, launches = [], []
    for budget in (1000000, 5):
        prob, agent, envs, run = learner_run(env, dev0, budget, frirl_amd.ExpectRows(E, dev0, expected=col))
        torch.cuda.synchronize()
        st = learner_state(prob, envs, run)
        st.pop("work")
        outs.append(st)
        launches.append(run.launches)
    print(env, "launches", launches)
    assert launches[1] > 10 * launches[0] and launches[1] > max(er.agent_run(env, e, er.mode_of(col[e]))["total_steps"] for e in range(E)) // 24
    assert_same(outs[0], outs[1], "budget 5")


@gpu
def test_expect_rows_beside_hyper_parameter_rows():
    """explore_rows_cases' acrobot cross case (hyper-parameter set e mod 6, exploration set e mod 4) with the flags of
    expect_ref.cross_column (e mod 2: every flagged agent is admitted, tests/test_expect_ref.py) and no target struct, three structs in
    one frirl_hip_learn_train_expect: every agent against the chain with all three applied."""
    import torch
    from tests import hparam_rows_cases as rc
    env, E = xc.CROSS_ENV, xc.CROSS_E
    seed, N = xc.CASES[env][2], xc.CROSS_EPISODES
    dev0 = torch.device("cuda", 0)
    pairs = xc.cross_sets()
    col = er.cross_column()
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=seed, env_id_base=xc.ID_BASE)
    rows = frirl_amd.HparamRows(E, dev0, **rc.columns([hc.demo_desc(env, name) for name, _ in pairs]))
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns([x for _, x in pairs]))
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=N, budget=700, rows=rows, explore=explore, expect=frirl_amd.ExpectRows(E, dev0, expected=col))
    torch.cuda.synchronize()
    for e in range(E):
        check_against_chain(er.cross_run(e, er.mode_of(col[e])), e, prob, envs, run)


# ---- 2. equivalences -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env", er.DEMOS)
def test_no_flag_is_the_target_call_and_a_greedy_expectation_the_plain_one(env):
    """frirl_hip_learn_train_target (mixed target column) against frirl_hip_learn_train_expect with the same other structs and an
    all-zero column, expected_all 0 and a NULL struct, on the exploring case: every state array byte for byte the same.  All agents
    expected with a target column of all Q against the same with all SARSA: the same bytes, the byte is not consulted.  Then, with
    no_random = 1 and no rows, expected_all 1 and an all-ones column against frirl_hip_learn_train: the same again."""
    import torch
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    E = xc.CASES[env][0]
    dev0 = torch.device("cuda", 0)
    forms = [None, frirl_amd.ExpectRows(E, dev0, expected=np.zeros(E, dtype=np.uint8)), frirl_amd.ExpectRows(E, dev0, expected_all=0), frirl_amd.ExpectRows.null(E)]
    outs = []
    for expect in forms:
        prob, agent, envs, run = learner_run(env, dev0, 700, expect, target=frirl_amd.TargetRows(E, dev0, target=tr.mixed_column(env)))
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the exploration sets were meant to desynchronise the agents"
    for o, what in zip(outs[1:], ("all-zero column", "expected_all 0", "NULL expect struct")):
        assert_same(outs[0], o, what)
    sides = []
    for t in (tr.Q, tr.SARSA):
        prob, agent, envs, run = learner_run(env, dev0, 700, frirl_amd.ExpectRows(E, dev0, expected_all=1), target=frirl_amd.TargetRows(E, dev0, target=np.full(E, t, dtype=np.uint8)))
        torch.cuda.synchronize()
        sides.append(learner_state(prob, envs, run))
    assert_same(sides[0], sides[1], "all expected: target Q against target SARSA")
    d = hc.demo_desc(env, "default")
    rng = np.random.default_rng(17)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))).to(dev0)
    outs = []
    for kw in (dict(), dict(expect=frirl_amd.ExpectRows(E, dev0, expected_all=1)), dict(expect=frirl_amd.ExpectRows(E, dev0, expected=np.ones(E, dtype=np.uint8)))):
        prob, agent, envs = frirl_amd.fresh_batch(d, E, xc.MAXR, dev0, start_states=start, no_random=1)
        run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=tr.EPISODES[env] + 1, budget=700, **kw)
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the start states were meant to desynchronise the agents"
    assert_same(outs[0], outs[1], "expected_all 1, greedy")
    assert_same(outs[0], outs[2], "all-ones column, greedy")


# ---- 3. caller-stepped agents ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("taught", [False, True], ids=["untaught", "taught"])
@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_caller_stepped_agents_learn_towards_the_expectation(nant, A, taught):
    """16 agents, 5 episodes of the torch point environment through frirl_hip_agent_begin_explore / frirl_hip_agent_observe_expect, agent
    e with epsilon 0.4 over a horizon of e mod 4 episodes and flag (e // 4) mod 2, with and without a scripted teacher that names the
    action at two steps in three, against expect_ref.ExpectMirror.  A taught flagged row takes the teacher's action and learns towards
    the expectation under its own rate.  A pick may follow the device only inside Mirror.pick's 1e-12 tie of the oracle, at most 10 % of
    the shape's picks; consequents at 1e-9."""
    import torch
    d = xc.point_description(nant, A)
    env, starts, mirrors = er.point_mirrors(nant, A, taught)
    E, maxR = xc.POINT_E, xc.POINT_MAXR
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV, no_random=0, seed=xc.POINT_SEED, env_id_base=xc.ID_BASE)
    explore = frirl_amd.ExploreRows(E, DEV, **xc.columns(xc.point_pairs()))
    expect = frirl_amd.ExpectRows(E, DEV, expected=er.point_flags())
    conv = frirl_amd.Convergence(prob, DEV)
    ss = torch.from_numpy(starts).to(DEV)

    def teacher(step):
        if not taught:
            return None
        return torch.tensor([tr.scripted_teacher(e, A)(step) for e in range(E)], dtype=torch.int32, device=DEV)

    for ep in range(xc.POINT_EPISODES):
        _, aidx = frirl_amd.agent_begin(prob, agent, envs, ss, explore=explore, teacher=teacher(0))
        envs.done.copy_(torch.maximum(envs.done, conv.converged))          # converged agents sit the episode out (frirl_amd.train)
        chosen = [aidx.clone()]
        live = [(envs.done == 0).clone()]
        action = agent.grid_values[nant - 1][aidx.long()]
        for t in range(d["max_steps"]):
            obs, reward, success = env.step(torch, envs.states, action)
            nxt, nidx = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32), explore=explore, expect=expect,
                                                teacher=teacher(t + 1))
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
            actions, steps, total = m.target_episode(env, [int(p[e]) for p in picks], ep + 1)
            got = [int(picks[t][e]) for t in range(len(actions))]
            assert got == actions, (nant, A, ep, e)
            assert int(envs.ep_steps[e]) == steps and float(envs.ep_reward[e]) == total and int(envs.done[e]) == 1
            R = m.five.R
            assert int(nrules[e]) == R, (nant, A, ep, e, m.expected)
            assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all()
            q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
            assert (np.abs(q - ref) <= TOL * np.maximum(np.abs(ref), 1e-9)).all(), (nant, A, ep, e, m.expected)
            assert int(envs.fus[e]) == int(m.fus)
            assert int(conv.converged[e]) == int(m.converged), (nant, A, ep, e)
    ties, picks_made = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, taught, "ties", ties, "picks", picks_made, "value differs", [m.value_differs for m in mirrors], "taught", sum(m.taught for m in mirrors))
    assert ties * 10 <= picks_made, (ties, picks_made)
    assert sum(m.value_differs for m in mirrors if m.expected) >= 10
    assert taught == (sum(m.taught for m in mirrors) > 0)


@gpu
def test_no_flag_is_the_target_call():
    """frirl_hip_agent_observe_expect with a NULL struct, an all-zero one and an all-zero column against frirl_hip_agent_observe_target
    (a mixed target column) on twin batches that explore at the agent's epsilon under a teacher, 30 steps of the point environment: the
    same bytes after every call.  An all-expected twin leaves them (it learns towards another value)."""
    import torch
    from tests.test_hip_external import PointEnv, assert_same, point_desc, state_arrays
    nant, A, E = 4, 5, 64
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    ss = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(9).uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    explore = frirl_amd.ExploreRows(E, DEV)
    target = frirl_amd.TargetRows(E, DEV, target=np.arange(E, dtype=np.uint8) % 2)
    sides = [dict(), dict(expect=frirl_amd.ExpectRows.null(E)), dict(expect=frirl_amd.ExpectRows(E, DEV)),
             dict(expect=frirl_amd.ExpectRows(E, DEV, expected=np.zeros(E, dtype=np.uint8))), dict(expect=frirl_amd.ExpectRows(E, DEV, expected_all=1))]
    batches = [frirl_amd.fresh_batch(d, E, 512, DEV, epsilon=0.25, no_random=0, seed=99, env_id_base=5) for _ in sides]
    acts = [frirl_amd.agent_begin(p, a, ev, ss, explore=explore)[0] for (p, a, ev) in batches]
    x_differs = False
    for t in range(30):
        teacher = torch.tensor([(t + e) % A if e % 2 else -1 for e in range(E)], dtype=torch.int32, device=DEV)
        for i, ((p, a, ev), kw) in enumerate(zip(batches, sides)):
            o, r, s = env.step(torch, ev.states, acts[i])
            n, _ = frirl_amd.agent_observe(p, a, ev, o.contiguous(), r.contiguous(), s.to(torch.int32), explore=explore, target=target, teacher=teacher, **kw)
            acts[i] = torch.where(ev.done == 0, n, acts[i])
        for (p, a, ev) in batches[1:4]:
            assert_same(state_arrays(batches[0][0], batches[0][2]), state_arrays(p, ev), t)
        x_differs = x_differs or not torch.equal(batches[0][0].rb, batches[4][0].rb)
    assert int(batches[0][0].nrules.max()) > 2 ** nant
    assert x_differs, "under exploration the expectation must learn other values than SARSA and Q"


@gpu
def test_a_flagged_row_that_may_not_explore_learns_towards_the_greedy_conclusion():
    """agent->no_random == 1 with a nonzero epsilon (the agent's own and an epsilon column): the rate of the expectation is 0, so
    frirl_hip_agent_observe_expect with every row flagged is frirl_hip_agent_observe_target with every row under target Q, byte for byte
    after every call -- under a teacher, so that the action taken differs from the greedy one and the SARSA twin leaves them."""
    import torch
    from tests.test_hip_external import PointEnv, assert_same, point_desc, state_arrays
    nant, A, E = 4, 5, 64
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    ss = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(9).uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    explore = frirl_amd.ExploreRows(E, DEV, epsilon=np.full(E, 0.3))
    sides = [dict(target=frirl_amd.TargetRows(E, DEV, target_all=tr.Q)), dict(expect=frirl_amd.ExpectRows(E, DEV, expected_all=1)),
             dict(expect=frirl_amd.ExpectRows(E, DEV, expected=np.ones(E, dtype=np.uint8)), target=frirl_amd.TargetRows(E, DEV, target_all=tr.SARSA)), dict()]
    batches = [frirl_amd.fresh_batch(d, E, 512, DEV, epsilon=0.25, no_random=1, seed=99, env_id_base=5) for _ in sides]
    acts = [frirl_amd.agent_begin(p, a, ev, ss, explore=explore)[0] for (p, a, ev) in batches]
    sarsa_differs = False
    for t in range(30):
        teacher = torch.tensor([(t + e) % A if e % 2 else -1 for e in range(E)], dtype=torch.int32, device=DEV)
        for i, ((p, a, ev), kw) in enumerate(zip(batches, sides)):
            o, r, s = env.step(torch, ev.states, acts[i])
            n, _ = frirl_amd.agent_observe(p, a, ev, o.contiguous(), r.contiguous(), s.to(torch.int32), explore=explore, teacher=teacher, **kw)
            acts[i] = torch.where(ev.done == 0, n, acts[i])
        for (p, a, ev) in batches[1:3]:
            assert_same(state_arrays(batches[0][0], batches[0][2]), state_arrays(p, ev), t)
        sarsa_differs = sarsa_differs or not torch.equal(batches[0][0].rb, batches[3][0].rb)
    assert int(batches[0][0].nrules.max()) > 2 ** nant
    assert sarsa_differs, "under a teacher Q(s', g) must differ from Q(s', a') somewhere: the twins would not tell the branch"


# ---- 4. batch object and demo --------------------------------------------------------------------------------------------------------
@gpu
def test_batch_object_trains_under_an_expected_column():
    """Twelve acrobot agents of a library-owned batch (greedy itself, no_random = 1) through frirl_hip_batch_set_exploration,
    frirl_hip_batch_set_expected and frirl_hip_batch_train: frirl_hip_batch_agent_report gives every agent the verdict, episodes, rules
    and last episode of the chain of its own mode.  frirl_hip_batch_get_expected returns what was set.  While the column is set the four
    calls that do not honour it refuse, naming themselves, and a rejected set leaves it in place; (NULL, 0) clears."""
    lib = frirl_amd.lib()
    env = "acrobot"
    E = xc.CASES[env][0]
    N = tr.EPISODES[env] + 1
    col = er.mixed_column(env)
    batch = frirl_amd.demo_batch_object(env, E, xc.MAXR, seed=er.SEEDS[env], env_id_base=xc.ID_BASE)
    try:
        assert (frirl_amd.batch_get_expected(batch) == 0).all()
        frirl_amd.batch_set_exploration(batch, **xc.columns(xc.agent_sets(env)))
        frirl_amd.batch_set_expected(batch, col)
        assert (frirl_amd.batch_get_expected(batch) == col).all()
        ran = C.c_int32(0)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, N, C.byref(ran)), "frirl_hip_batch_train")
        rep = frirl_amd.batch_agent_report(batch)
        runs = [er.agent_run(env, e, er.mode_of(col[e])) for e in range(E)]
        for e in range(E):
            _report_matches(rep, e, runs[e])
        assert ran.value == max(r["episodes"] for r in runs)
        frirl_amd.batch_set_exploration(batch, clear=True)                 # the column alone refuses too
        assert lib.frirl_hip_batch_episode(batch) == -2 and b"frirl_hip_batch_episode" in lib.frirl_hip_last_error() and b"expected" in lib.frirl_hip_last_error()
        res = frirl_amd.TeachResult()
        assert lib.frirl_hip_batch_teach(batch, 0, 1, None, 1, None, C.byref(res)) == -2 and b"frirl_hip_batch_teach" in lib.frirl_hip_last_error()
        assert lib.frirl_hip_batch_merge_round(batch, None) == -2 and b"frirl_hip_batch_merge_round" in lib.frirl_hip_last_error()
        epr, rounds = C.c_int32(0), C.c_int32(0)
        assert lib.frirl_hip_batch_train_merged(batch, 4, 2, C.byref(epr), C.byref(rounds)) == -2 and b"frirl_hip_batch_train_merged" in lib.frirl_hip_last_error()
        with pytest.raises(frirl_amd.FrirlHipError, match="agent 4.*expected"):
            frirl_amd.batch_set_expected(batch, [0] * 4 + [2] + [0] * (E - 5))
        with pytest.raises(frirl_amd.FrirlHipError, match="expected_all"):
            frirl_amd.batch_set_expected(batch, None, 3)
        assert (frirl_amd.batch_get_expected(batch) == col).all(), "a rejected set must leave the batch as it was"
        assert lib.frirl_hip_batch_episode(batch) == -2
        frirl_amd.batch_set_expected(batch, None, 1)                       # expected_all alone: no column
        assert (frirl_amd.batch_get_expected(batch) == 1).all() and lib.frirl_hip_batch_episode(batch) == -2
        frirl_amd.batch_set_expected(batch)                                # clear
        assert (frirl_amd.batch_get_expected(batch) == 0).all() and lib.frirl_hip_batch_episode(batch) == 0
    finally:
        lib.frirl_hip_batch_destroy(batch)


@gpu
def test_batch_clone_gathers_a_set_expected_column():
    """frirl_hip_batch_clone with inherit_rows: a cloned agent takes its source's flag with its other set columns; without inherit_rows
    it keeps its own; with expected_all alone there is no column and nothing to gather."""
    lib = frirl_amd.lib()
    env, E = "mountaincar", 6
    col = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8)
    src = np.array([0, 1, 2, 3, 1, 0], dtype=np.int32)                     # agent 4 <- 1 (expected), agent 5 <- 0 (not)
    batch = frirl_amd.demo_batch_object(env, E, xc.MAXR, seed=er.SEEDS[env], env_id_base=xc.ID_BASE)
    try:
        frirl_amd.batch_set_exploration(batch, epsilon=np.linspace(0.0, 0.5, E))
        frirl_amd.batch_set_expected(batch, col)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, 3, None), "frirl_hip_batch_train")
        assert frirl_amd.batch_clone(batch, src, inherit_rows=False) == 2
        assert (frirl_amd.batch_get_expected(batch) == col).all()
        assert frirl_amd.batch_clone(batch, src, inherit_rows=True) == 2
        assert frirl_amd.batch_get_expected(batch).tolist() == [0, 1, 0, 1, 1, 0]
        assert np.array_equal(frirl_amd.batch_get_exploration(batch)["epsilon"], np.linspace(0.0, 0.5, E)[src])
        frirl_amd.batch_set_expected(batch, None, 1)
        assert frirl_amd.batch_clone(batch, src, inherit_rows=True) == 2
        assert (frirl_amd.batch_get_expected(batch) == 1).all()
        frirl_amd.check(lib.frirl_hip_batch_train(batch, 5, None), "frirl_hip_batch_train")     # training goes on after a clone
    finally:
        lib.frirl_hip_batch_destroy(batch)


@gpu
def test_demo_reports_the_expected_rows(tmp_path):
    """frirl_demo --env acrobot --agents 12 --explore x.txt --expected-rows f.txt --seed 1234 --id-base 77 --max-episodes 10: the `batch`
    line ends in the choice, and the `explore` lines carry the counts and means of the chains of each agent's own mode."""
    env = "acrobot"
    E, sets, _, _ = xc.CASES[env]
    N = tr.EPISODES[env] + 1
    col = er.mixed_column(env)
    x, t = tmp_path / "x.txt", tmp_path / "f.txt"
    x.write_text("# epsilon horizon\n" + "".join(f"{eps!r} {h}\n" for eps, h in sets))
    t.write_text("# flag of agent e: line e mod 12\n" + "".join(f"{int(v)}\n" for v in col))
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    r = subprocess.run([demo, "--env", env, "--agents", str(E), "--seed", str(er.SEEDS[env]), "--max-episodes", str(N), "--explore", str(x), "--expected-rows", str(t),
                        "--id-base", str(xc.ID_BASE)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    runs = [er.agent_run(env, e, er.mode_of(col[e])) for e in range(E)]
    batch = [l for l in r.stdout.splitlines() if l.startswith(f"batch {env}: ")]
    assert len(batch) == 1 and batch[0].endswith(f" expected rows ({int(col.sum())} of {E} agents expected)"), r.stdout
    m = re.match(rf"batch {env}: agents (\d+) episodes (\d+) converged (\d+) env-steps (\d+) ", batch[0])
    assert m and (int(m[1]), int(m[2]), int(m[3]), int(m[4])) == (E, max(x["episodes"] for x in runs), sum(x["converged"] for x in runs), sum(x["total_steps"] for x in runs)), batch[0]
    lines = [l for l in r.stdout.splitlines() if l.startswith(f"explore {env}: line ")]
    assert len(lines) == len(sets), r.stdout
    for s, line in enumerate(lines):
        m = re.match(rf"explore {env}: line (\d+) agents (\d+) converged (\d+) mean-episodes ([\d.]+) max-episodes (\d+) mean-rules ([\d.]+) mean-reward (-?[\d.]+)$", line)
        assert m, line
        mine = runs[s::len(sets)]
        assert (int(m[1]), int(m[2]), int(m[3]), int(m[5])) == (s, len(mine), sum(x["converged"] for x in mine), max(x["episodes"] for x in mine)), line
        assert abs(float(m[6]) - np.mean([x["fr"].five.R for x in mine])) <= 6e-4, line
        reward = np.mean([x["ep_reward"] for x in mine])
        assert abs(float(m[7]) - reward) <= 1e-6 * max(1.0, abs(reward)), line
    r = subprocess.run([demo, "--env", env, "--agents", "3", "--max-episodes", "4", "--expected"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and any(l.startswith(f"batch {env}: ") and l.endswith(" expected all") for l in r.stdout.splitlines()), (r.stdout, r.stderr)
