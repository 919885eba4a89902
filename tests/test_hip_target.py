"""Per-agent TD target (frirl_hip_target_rows) on the device: a launch in which agent e learns towards Q(s', a') of the action it takes
(SARSA) or towards Q(s', g) of the greedy action its pick started from (Q), against the construct loop restated from the oracle's
pieces (tests/target_ref.py).  The cases and the conditions under which they tell one target from the other are asserted on the CPU
by tests/test_target_ref.py.

1. the persistent learner (frirl_hip_learn_train_target) per agent against its chain: every lane-group size, launch boundaries inside
   episodes, crossed with hyper-parameter rows
2. equivalences: an all-SARSA column, target_all 0 and a NULL struct are frirl_hip_learn_train_explore; all-Q without exploration is
   frirl_hip_learn_train
3. caller-stepped agents (frirl_hip_agent_observe_target) against per-agent mirrors, taught and untaught; NULL = the _explore call
4. the batch object (frirl_hip_batch_set_target / _get_target, clone with inherit_rows) and frirl_demo --target-rows

Bars: decisions, counters, reward bits, appended antecedents exact; consequents <= 1e-9 relative (the bar of
tests/test_hip_explore_rows.py for the same comparison).
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
from tests import target_ref as tr

DEV = "cuda"
TOL = 1e-9
gpu = pytest.mark.gpu


def check_against_chain(r, e, prob, envs, run):
    """Agent e of a finished learner run against its chain r (target_ref.chain)."""
    from tests.test_hip_learn import check_agent_against_oracle
    got = (int(run.conv.converged[e]), int(run.conv.episodes[e]), int(run.steps_total[e]))
    assert got == (r["converged"], r["episodes"], r["total_steps"]), (e, got, (r["converged"], r["episodes"], r["total_steps"]))
    assert int(envs.ep_steps[e]) == r["ep_steps"] and xc.bits(float(envs.ep_reward[e])) == xc.bits(r["ep_reward"]), e
    assert int(envs.fus[e]) == int(r["fr"].fus), e
    check_agent_against_oracle(r["fr"], prob, envs, e)


def differs_from(r, e, prob):
    """The device's rule base of agent e is NOT the chain r's: another rule count, or a consequent further than 1e-6 relative (the
    contract's bound, a thousand times the bar of the comparison above)."""
    f = r["fr"].five
    R = f.R
    if int(prob.nrules[e]) != R:
        return True
    q = prob.rb[e, prob.nant, :R].cpu().numpy()
    return bool((np.abs(q - f.rconc[:R]) > 1e-6 * np.maximum(np.abs(f.rconc[:R]), 1e-9)).any())


def learner_run(env, dev0, budget, target=None, **kw):
    E, sets, seed, _ = xc.CASES[env]
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=seed, env_id_base=xc.ID_BASE)
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns(xc.agent_sets(env)))
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=tr.EPISODES[env] + 1, budget=budget, explore=explore, target=target, **kw)
    return prob, agent, envs, run


# ---- 1. the persistent learner -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env,slices", [(env, s) for env in tr.DEMOS for s in (0, 1, 4, 64)])
def test_persistent_learner_follows_each_agents_chain_under_its_own_target(env, slices, hip_option):
    """The agents of explore_rows_cases.CASES over 8 / 9 / 7 episodes with a mixed target column (every (epsilon, horizon) set under both
    targets) through frirl_hip_learn_train_target, at the default lane-group size and at 1, 4 and 64 rule slices.  Every agent follows
    the chain of its own target; every exploring agent under target Q does NOT end where its SARSA chain ends -- without the feature
    it would."""
    import torch
    E, sets, seed, _ = xc.CASES[env]
    dev0 = torch.device("cuda", 0)
    if slices:
        hip_option("learn_slices", slices)
    col = tr.mixed_column(env)
    prob, agent, envs, run = learner_run(env, dev0, 700, frirl_amd.TargetRows(E, dev0, target=col))
    torch.cuda.synchronize()
    told_apart = 0
    for e in range(E):
        check_against_chain(tr.agent_run(env, e, int(col[e])), e, prob, envs, run)
        if col[e] == tr.Q and sets[e % len(sets)][0] > 0:
            assert differs_from(tr.agent_run(env, e, tr.SARSA), e, prob), (e, "an exploring agent under target Q ended on its SARSA chain")
            told_apart += 1
    assert told_apart >= len(sets) - 1


@gpu
@pytest.mark.parametrize("env", ["acrobot", "cartpole"])
def test_launch_boundaries_inside_episodes_change_nothing(env):
    """The same run with a budget of 5 steps per launch -- every launch boundary falls inside an episode, and the queue re-sorts the
    agents between launches, so a target taken by launch slot would be another agent's -- against one with a budget no agent exhausts:
    every state array byte for byte the same (the rule-visit counters, a profiling aid, apart)."""
    import torch
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    E = xc.CASES[env][0]
    dev0 = torch.device("cuda", 0)
    outs, launches = [], []
    for budget in (1000000, 5):
        prob, agent, envs, run = learner_run(env, dev0, budget, frirl_amd.TargetRows(E, dev0, target=tr.mixed_column(env)))
        torch.cuda.synchronize()
        st = learner_state(prob, envs, run)
        st.pop("work")
        outs.append(st)
        launches.append(run.launches)
    print(env, "launches", launches)
    assert launches[1] > 10 * launches[0] and launches[1] > max(tr.agent_run(env, e, int(tr.mixed_column(env)[e]))["total_steps"] for e in range(E)) // 24
    assert_same(outs[0], outs[1], "budget 5")


@gpu
def test_target_rows_beside_hyper_parameter_rows():
    """explore_rows_cases' acrobot cross case (hyper-parameter set e mod 6, exploration set e mod 4) with target e mod 2, all three
    structs in one frirl_hip_learn_train_target: every agent against the chain with all three applied."""
    import torch
    from tests import hparam_rows_cases as rc
    env, E = xc.CROSS_ENV, xc.CROSS_E
    seed, N = xc.CASES[env][2], xc.CROSS_EPISODES
    dev0 = torch.device("cuda", 0)
    pairs = xc.cross_sets()
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, xc.MAXR, dev0, no_random=0, seed=seed, env_id_base=xc.ID_BASE)
    rows = frirl_amd.HparamRows(E, dev0, **rc.columns([hc.demo_desc(env, name) for name, _ in pairs]))
    explore = frirl_amd.ExploreRows(E, dev0, **xc.columns([x for _, x in pairs]))
    target = frirl_amd.TargetRows(E, dev0, target=tr.cross_column())
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=N, budget=700, rows=rows, explore=explore, target=target)
    torch.cuda.synchronize()
    for e in range(E):
        check_against_chain(tr.cross_run(e), e, prob, envs, run)


# ---- 2. equivalences -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env", tr.DEMOS)
def test_a_sarsa_target_is_the_explore_call_and_a_greedy_q_target_the_plain_one(env):
    """frirl_hip_learn_train_explore against frirl_hip_learn_train_target with an all-zero column, with target_all 0 and with a NULL
    struct, on the exploring case: every state array byte for byte the same.  Then, with no_random = 1 and no rows, target_all Q and an
    all-ones column against frirl_hip_learn_train: the same again -- without exploration the two targets coincide bit for bit."""
    import torch
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    E = xc.CASES[env][0]
    dev0 = torch.device("cuda", 0)
    forms = [None, frirl_amd.TargetRows(E, dev0, target=np.zeros(E, dtype=np.uint8)), frirl_amd.TargetRows(E, dev0, target_all=tr.SARSA), frirl_amd.TargetRows.null(E)]
    outs = []
    for target in forms:
        prob, agent, envs, run = learner_run(env, dev0, 700, target)
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the exploration sets were meant to desynchronise the agents"
    for o, what in zip(outs[1:], ("all-SARSA column", "target_all SARSA", "NULL target struct")):
        assert_same(outs[0], o, what)
    d = hc.demo_desc(env, "default")
    rng = np.random.default_rng(17)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))).to(dev0)
    outs = []
    for kw in (dict(), dict(target=frirl_amd.TargetRows(E, dev0, target_all=tr.Q)), dict(target=frirl_amd.TargetRows(E, dev0, target=np.ones(E, dtype=np.uint8)))):
        prob, agent, envs = frirl_amd.fresh_batch(d, E, xc.MAXR, dev0, start_states=start, no_random=1)
        run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=tr.EPISODES[env] + 1, budget=700, **kw)
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the start states were meant to desynchronise the agents"
    assert_same(outs[0], outs[1], "target_all Q, greedy")
    assert_same(outs[0], outs[2], "all-Q column, greedy")


# ---- 3. caller-stepped agents ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("taught", [False, True], ids=["untaught", "taught"])
@pytest.mark.parametrize("nant,A", xc.POINT_SHAPES)
def test_caller_stepped_agents_learn_towards_their_own_target(nant, A, taught):
    """16 agents, 5 episodes of the torch point environment through frirl_hip_agent_begin_explore / frirl_hip_agent_observe_target, agent
    e with epsilon 0.4 over a horizon of e mod 4 episodes and target (e // 4) mod 2, with and without a scripted teacher that names the
    action at two steps in three, against target_ref.TargetMirror.  A taught row under target Q takes the teacher's action and learns
    towards Q(s', g).  A pick may follow the device only inside Mirror.pick's 1e-12 tie of the oracle, at most 10 % of the shape's picks;
    consequents at 1e-9."""
    import torch
    d = xc.point_description(nant, A)
    env, starts, mirrors = tr.point_mirrors(nant, A, taught)
    E, maxR = xc.POINT_E, xc.POINT_MAXR
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV, no_random=0, seed=xc.POINT_SEED, env_id_base=xc.ID_BASE)
    explore = frirl_amd.ExploreRows(E, DEV, **xc.columns(xc.point_pairs()))
    target = frirl_amd.TargetRows(E, DEV, target=tr.point_targets())
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
            nxt, nidx = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32), explore=explore, target=target,
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
            assert int(nrules[e]) == R, (nant, A, ep, e, m.target)
            assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all()
            q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
            assert (np.abs(q - ref) <= TOL * np.maximum(np.abs(ref), 1e-9)).all(), (nant, A, ep, e, m.target)
            assert int(envs.fus[e]) == int(m.fus)
            assert int(conv.converged[e]) == int(m.converged), (nant, A, ep, e)
    ties, picks_made = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, taught, "ties", ties, "picks", picks_made, "g != a'", [m.off_policy for m in mirrors], "taught", sum(m.taught for m in mirrors))
    assert ties * 10 <= picks_made, (ties, picks_made)
    assert sum(m.off_policy for m in mirrors if m.target == tr.Q) >= 10
    assert taught == (sum(m.taught for m in mirrors) > 0)


@gpu
def test_no_target_is_the_explore_call():
    """frirl_hip_agent_observe_target with a NULL target struct, an all-zero one and an all-zero column against
    frirl_hip_agent_observe_explore on twin batches that explore at the agent's epsilon under a teacher, 30 steps of the point
    environment: the same bytes after every call.  An all-Q twin leaves them (it learns towards another value)."""
    import torch
    from tests.test_hip_external import PointEnv, assert_same, point_desc, state_arrays
    nant, A, E = 4, 5, 64
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    ss = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(9).uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    explore = frirl_amd.ExploreRows(E, DEV)
    sides = [dict(), dict(target=frirl_amd.TargetRows.null(E)), dict(target=frirl_amd.TargetRows(E, DEV)),
             dict(target=frirl_amd.TargetRows(E, DEV, target=np.zeros(E, dtype=np.uint8))), dict(target=frirl_amd.TargetRows(E, DEV, target_all=tr.Q))]
    batches = [frirl_amd.fresh_batch(d, E, 512, DEV, epsilon=0.25, no_random=0, seed=99, env_id_base=5) for _ in sides]
    acts = [frirl_amd.agent_begin(p, a, ev, ss, explore=explore)[0] for (p, a, ev) in batches]
    q_differs = False
    for t in range(30):
        teacher = torch.tensor([(t + e) % A if e % 2 else -1 for e in range(E)], dtype=torch.int32, device=DEV)
        for i, ((p, a, ev), kw) in enumerate(zip(batches, sides)):
            o, r, s = env.step(torch, ev.states, acts[i])
            n, _ = frirl_amd.agent_observe(p, a, ev, o.contiguous(), r.contiguous(), s.to(torch.int32), explore=explore, teacher=teacher, **kw)
            acts[i] = torch.where(ev.done == 0, n, acts[i])
        for (p, a, ev) in batches[1:4]:
            assert_same(state_arrays(batches[0][0], batches[0][2]), state_arrays(p, ev), t)
        q_differs = q_differs or not torch.equal(batches[0][0].rb, batches[4][0].rb)
    assert int(batches[0][0].nrules.max()) > 2 ** nant
    assert q_differs, "under a teacher and exploration target Q must learn other values than SARSA"


# ---- 4. batch object and demo --------------------------------------------------------------------------------------------------------
def _report_matches(rep, e, r):
    got = (int(rep["converged"][e]), int(rep["episodes"][e]), int(rep["rules"][e]), int(rep["ep_steps"][e]), xc.bits(rep["ep_reward"][e]))
    assert got == (r["converged"], r["episodes"], r["fr"].five.R, r["ep_steps"], xc.bits(r["ep_reward"])), (e, got)


@gpu
def test_batch_object_trains_under_a_target_column():
    """Twelve acrobot agents of a library-owned batch (greedy itself, no_random = 1) through frirl_hip_batch_set_exploration,
    frirl_hip_batch_set_target and frirl_hip_batch_train: frirl_hip_batch_agent_report gives every agent the verdict, episodes, rules and
    last episode of the chain of its own target, as the primitive does.  frirl_hip_batch_get_target returns what was set.  While a
    target is set the four calls that do not honour it refuse, naming themselves, and a rejected set leaves it in place; target_all Q
    alone (no exploration: greedy) trains as the plain batch does."""
    lib = frirl_amd.lib()
    env = "acrobot"
    E, sets, seed, _ = xc.CASES[env]
    N = tr.EPISODES[env] + 1
    col = tr.mixed_column(env)
    batch = frirl_amd.demo_batch_object(env, E, xc.MAXR, seed=seed, env_id_base=xc.ID_BASE)
    try:
        assert (frirl_amd.batch_get_target(batch) == 0).all()
        frirl_amd.batch_set_exploration(batch, **xc.columns(xc.agent_sets(env)))
        frirl_amd.batch_set_target(batch, col)
        assert (frirl_amd.batch_get_target(batch) == col).all()
        ran = C.c_int32(0)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, N, C.byref(ran)), "frirl_hip_batch_train")
        rep = frirl_amd.batch_agent_report(batch)
        for e in range(E):
            _report_matches(rep, e, tr.agent_run(env, e, int(col[e])))
        assert ran.value == max(tr.agent_run(env, e, int(col[e]))["episodes"] for e in range(E))
        frirl_amd.batch_set_exploration(batch, clear=True)                 # the target alone refuses too
        assert lib.frirl_hip_batch_episode(batch) == -2 and b"frirl_hip_batch_episode" in lib.frirl_hip_last_error() and b"target" in lib.frirl_hip_last_error()
        res = frirl_amd.TeachResult()
        assert lib.frirl_hip_batch_teach(batch, 0, 1, None, 1, None, C.byref(res)) == -2 and b"frirl_hip_batch_teach" in lib.frirl_hip_last_error()
        assert lib.frirl_hip_batch_merge_round(batch, None) == -2 and b"frirl_hip_batch_merge_round" in lib.frirl_hip_last_error()
        er, rounds = C.c_int32(0), C.c_int32(0)
        assert lib.frirl_hip_batch_train_merged(batch, 4, 2, C.byref(er), C.byref(rounds)) == -2 and b"frirl_hip_batch_train_merged" in lib.frirl_hip_last_error()
        with pytest.raises(frirl_amd.FrirlHipError, match="agent 4.*target"):
            frirl_amd.batch_set_target(batch, [0] * 4 + [2] + [0] * (E - 5))
        with pytest.raises(frirl_amd.FrirlHipError, match="target_all"):
            frirl_amd.batch_set_target(batch, None, 3)
        assert (frirl_amd.batch_get_target(batch) == col).all(), "a rejected set must leave the batch as it was"
        assert lib.frirl_hip_batch_episode(batch) == -2
        frirl_amd.batch_set_target(batch, None, tr.Q)                      # target_all alone: no column
        assert (frirl_amd.batch_get_target(batch) == 1).all() and lib.frirl_hip_batch_episode(batch) == -2
        frirl_amd.batch_set_target(batch)                                  # clear
        assert (frirl_amd.batch_get_target(batch) == 0).all() and lib.frirl_hip_batch_episode(batch) == 0
    finally:
        lib.frirl_hip_batch_destroy(batch)
    # target_all Q on a greedy batch is the plain batch
    reports = []
    for q in (False, True):
        batch = frirl_amd.demo_batch_object(env, 3, xc.MAXR, seed=seed, env_id_base=xc.ID_BASE)
        try:
            if q:
                frirl_amd.batch_set_target(batch, None, tr.Q)
            frirl_amd.check(lib.frirl_hip_batch_train(batch, N, None), "frirl_hip_batch_train")
            reports.append(frirl_amd.batch_agent_report(batch))
        finally:
            lib.frirl_hip_batch_destroy(batch)
    for k in ("converged", "episodes", "rules", "ep_steps"):
        assert (reports[0][k] == reports[1][k]).all(), k
    assert reports[0]["ep_reward"].tobytes() == reports[1]["ep_reward"].tobytes()
    _report_matches(reports[1], 0, tr.agent_run(env, 0, tr.Q))              # set 0: epsilon 0


@gpu
def test_batch_clone_gathers_a_set_target_column():
    """frirl_hip_batch_clone with inherit_rows: a cloned agent takes its source's target with its other set columns; without inherit_rows
    it keeps its own; with target_all alone there is no column and nothing to gather."""
    lib = frirl_amd.lib()
    env, E = "mountaincar", 6
    col = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8)
    src = np.array([0, 1, 2, 3, 1, 0], dtype=np.int32)                     # agent 4 <- 1 (Q), agent 5 <- 0 (SARSA)
    batch = frirl_amd.demo_batch_object(env, E, xc.MAXR, seed=1265, env_id_base=xc.ID_BASE)
    try:
        frirl_amd.batch_set_exploration(batch, epsilon=np.linspace(0.0, 0.5, E))
        frirl_amd.batch_set_target(batch, col)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, 3, None), "frirl_hip_batch_train")
        assert frirl_amd.batch_clone(batch, src, inherit_rows=False) == 2
        assert (frirl_amd.batch_get_target(batch) == col).all()
        assert frirl_amd.batch_clone(batch, src, inherit_rows=True) == 2
        assert frirl_amd.batch_get_target(batch).tolist() == [0, 1, 0, 1, 1, 0]
        assert np.array_equal(frirl_amd.batch_get_exploration(batch)["epsilon"], np.linspace(0.0, 0.5, E)[src])
        frirl_amd.batch_set_target(batch, None, tr.Q)
        assert frirl_amd.batch_clone(batch, src, inherit_rows=True) == 2
        assert (frirl_amd.batch_get_target(batch) == 1).all()
        frirl_amd.check(lib.frirl_hip_batch_train(batch, 5, None), "frirl_hip_batch_train")     # training goes on after a clone
    finally:
        lib.frirl_hip_batch_destroy(batch)


@gpu
def test_demo_reports_the_target(tmp_path):
    """frirl_demo --env acrobot --agents 12 --explore x.txt --target-rows t.txt --seed 1234 --id-base 77 --max-episodes 10: the `batch`
    line ends in the target, and the `explore` lines carry the counts and means of the chains of each agent's own target."""
    env = "acrobot"
    E, sets, seed, _ = xc.CASES[env]
    N = tr.EPISODES[env] + 1
    col = tr.mixed_column(env)
    x, t = tmp_path / "x.txt", tmp_path / "t.txt"
    x.write_text("# epsilon horizon\n" + "".join(f"{eps!r} {h}\n" for eps, h in sets))
    t.write_text("# target of agent e: line e mod 12\n" + "".join(f"{int(v)}\n" for v in col))
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    r = subprocess.run([demo, "--env", env, "--agents", str(E), "--seed", str(seed), "--max-episodes", str(N), "--explore", str(x), "--target-rows", str(t),
                        "--id-base", str(xc.ID_BASE)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    runs = [tr.agent_run(env, e, int(col[e])) for e in range(E)]
    batch = [l for l in r.stdout.splitlines() if l.startswith(f"batch {env}: ")]
    assert len(batch) == 1 and batch[0].endswith(f" target rows ({int(col.sum())} of {E} agents q)"), r.stdout
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
    r = subprocess.run([demo, "--env", env, "--agents", "3", "--max-episodes", "4", "--target", "q"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and any(l.startswith(f"batch {env}: ") and l.endswith(" target q") for l in r.stdout.splitlines()), (r.stdout, r.stderr)
