"""Per-agent hyper-parameter rows (frirl_hip_hparam_rows) on the device: a launch in which agent e learns under its own alpha, gamma,
insertion bounds, spread threshold and skip_rules, against the oracle run of ITS set.  The sets, their oracle runs and the conditions
under which a mixed batch tells a wrong row from the right one are in tests/hparams_cases.py and tests/hparam_rows_cases.py, asserted
on the CPU by tests/test_hparam_rows_ref.py.

1. the persistent learner (frirl_hip_learn_train_rows) per agent against the oracle, several sets in one wave
2. rows equal to the agent's values: byte-identical to frirl_hip_learn_train
3. caller-stepped agents (frirl_hip_agent_begin_rows / _observe_rows) against per-agent mirrors; NULL columns = the taught call
4. the batch object (frirl_hip_batch_set_hparams / _agent_report) and frirl_demo --hparams

Bars: decisions, counters, reward bits, appended antecedents exact; consequents <= 1e-9 relative (the contract is 1e-6).
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

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
DEMOS = ["mountaincar", "acrobot", "cartpole"]


def demo_rows(env, E, device):
    """Agent e under set e mod nsets of the demo's mixed batch: (set name per agent, HparamRows)."""
    sets = rc.demo_sets(env)
    names = [sets[e % len(sets)] for e in range(E)]
    return names, frirl_amd.HparamRows(E, device, **rc.columns([hc.demo_desc(env, n) for n in names]))


# ---- 1. the persistent learner -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices,budget", [(0, 700), (1, 700), (64, 700), (0, 5)])
@pytest.mark.parametrize("env", DEMOS)
def test_persistent_learner_follows_each_agents_own_oracle(env, slices, budget, hip_option):
    """23 agents on the demo's own description, agent e under set e mod nsets (3 / 6 / 6 sets: one wave holds several sets and 23 is
    no multiple of anything), through frirl_hip_learn_train_rows for the default lane-group size and 1 and 64 rule slices at a budget
    of 700 steps, and at a budget of 5 (every launch boundary re-reads the rows; the queue re-sorts the agents by rule count between
    launches, so a row taken by launch slot would be another agent's).  Per agent against the oracle's run of its set: converged,
    episodes, total steps, the last episode's steps and reward bits, the sticky flag: exact; rule base: check_agent_against_oracle."""
    import torch
    from tests.test_hip_learn import check_agent_against_oracle
    E = 23
    dev0 = torch.device("cuda", 0)
    if slices:
        hip_option("learn_slices", slices)
    names, rows = demo_rows(env, E, dev0)
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, "default"), E, hc.TRAJ_MAXR, dev0)
    assert frirl_amd.learn_supported(prob, agent)
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=hc.TRAJ_EPISODES[env], budget=budget, rows=rows)
    torch.cuda.synchronize()
    converged, episodes, total = run.conv.converged.cpu().numpy(), run.conv.episodes.cpu().numpy(), run.steps_total.cpu().numpy()
    ep_steps, ep_reward, fus = envs.ep_steps.cpu().numpy(), envs.ep_reward.cpu().numpy(), envs.fus.cpu().numpy()
    for e, name in enumerate(names):
        r = hc.traj_run(env, name)
        fr = r["fr"]
        assert (int(converged[e]), int(episodes[e]), int(total[e])) == (r["converged"], r["episodes"], r["total_steps"]), (e, name, int(total[e]), r["total_steps"])
        assert int(ep_steps[e]) == fr.ep_steps and ep_reward[e].view(np.uint64) == np.float64(fr.ep_reward).view(np.uint64), (e, name)
        assert int(fus[e]) == int(fr.fus), (e, name)
        check_agent_against_oracle(fr, prob, envs, e)
    if budget == 5:
        assert run.launches > max(hc.traj_run(env, n)["total_steps"] for n in set(names)) // 24


# ---- 2. rows that repeat the agent's values ------------------------------------------------------------------------------------------
def learner_state(prob, envs, run):
    c = run.conv
    return dict(rb=prob.rb, nrules=prob.nrules, uidx=prob.uidx, rant=envs.rant, states=envs.states, q_ant=envs.q_ant, fus=envs.fus, done=envs.done,
                ep_steps=envs.ep_steps, ep_reward=envs.ep_reward, status=envs.status, episode=envs.episode, spread_ant=envs.spread_ant,
                spread_R=envs.spread_R, prev_nrules=c.prev_nrules, prev_steps=c.prev_steps, prev_reward=c.prev_reward, prev_rconc=c.prev_rconc,
                converged=c.converged, episodes=c.episodes, steps_total=run.steps_total, work=run.work)


@pytest.mark.parametrize("env", DEMOS)
def test_rows_equal_to_the_agents_values_change_nothing(env):
    """21 agents with start states spread over the state grids (never in step): frirl_hip_learn_train, then frirl_hip_learn_train_rows
    with all six columns filled with the agent's own values, then with the alpha column alone -- rule bases, counters, episode and
    convergence state byte for byte the same."""
    import torch
    from tests.test_hip_external import assert_same
    E = 21
    dev0 = torch.device("cuda", 0)
    d = hc.demo_desc(env, "default")
    rng = np.random.default_rng(17)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))).to(dev0)
    full = rc.columns([d] * E)
    outs = []
    for columns in (None, full, dict(alpha=full["alpha"])):
        prob, agent, envs = frirl_amd.fresh_batch(d, E, hc.TRAJ_MAXR, dev0, start_states=start)
        rows = None if columns is None else frirl_amd.HparamRows(E, dev0, **columns)
        run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=hc.TRAJ_EPISODES[env], budget=700, rows=rows)
        torch.cuda.synchronize()
        outs.append(learner_state(prob, envs, run))
    assert len(set(outs[0]["steps_total"].tolist())) > 3, "the start states were meant to desynchronise the agents"
    assert_same(outs[0], outs[1], "all six columns")
    assert_same(outs[0], outs[2], "alpha alone")


# ---- 3. caller-stepped agents ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nant,A", rc.POINT_SHAPES)
def test_caller_stepped_agents_follow_each_agents_own_oracle(nant, A):
    """tests/test_hip_external.py::follow_the_oracle's loop (16 agents, 4 episodes of the torch point environment) through
    frirl_hip_agent_begin_rows / _observe_rows, the Agent carrying the shape's own values and agent e learning under set
    (e + rotation) mod 8 of hparams_cases.SETS, against a mirror built on ITS set's description.  A pick may follow the device only
    inside Mirror.pick's 1e-12 tie of the oracle, at most 10 % of the shape's picks; consequents at 1e-9."""
    import torch
    d, env, starts, descs, mirrors = rc.point_case(nant, A)
    E, maxR = rc.POINT_E, rc.POINT_MAXR
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV)
    rows = frirl_amd.HparamRows(E, DEV, **rc.columns(descs))
    conv = frirl_amd.Convergence(prob, DEV)
    ss = torch.from_numpy(starts).to(DEV)
    for ep in range(rc.POINT_EPISODES):
        _, aidx = frirl_amd.agent_begin(prob, agent, envs, ss, rows=rows)
        envs.done.copy_(torch.maximum(envs.done, conv.converged))          # converged agents sit the episode out (frirl_amd.train)
        chosen = [aidx.clone()]
        live = [(envs.done == 0).clone()]
        action = agent.grid_values[nant - 1][aidx.long()]
        for t in range(d["max_steps"]):
            obs, reward, success = env.step(torch, envs.states, action)
            nxt, nidx = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32), rows=rows)
            chosen.append(nidx.clone())
            live.append((envs.done == 0).clone())
            action = torch.where(live[-2], nxt, action)
        conv.update(prob, agent, envs)      # reads reward_good_above and qdiff_final_tolerance only: per batch, the same in every set
        torch.cuda.synchronize()
        was_live = [l.cpu().numpy() for l in live]
        picks = [c.cpu().numpy() for c in chosen]
        rant, rb, nrules = envs.rant.cpu().numpy(), prob.rb.cpu().numpy(), prob.nrules.cpu().numpy()
        for e, m in enumerate(mirrors):
            if m.converged:
                assert not was_live[0][e] and int(conv.converged[e]) == 1
                continue
            actions, steps, total = m.episode(env, [int(p[e]) for p in picks])
            got = [int(picks[t][e]) for t in range(len(actions))]
            assert got == actions, (nant, A, ep, e)
            assert int(envs.ep_steps[e]) == steps and float(envs.ep_reward[e]) == total and int(envs.done[e]) == 1
            R = m.five.R
            assert int(nrules[e]) == R, (nant, A, ep, e, rc.point_sets(nant, A)[e])
            assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all()
            q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
            assert (np.abs(q - ref) <= TOL * np.maximum(np.abs(ref), 1e-9)).all(), (nant, A, ep, e, rc.point_sets(nant, A)[e])
            assert int(envs.fus[e]) == int(m.fus)
            assert int(conv.converged[e]) == int(m.converged), (nant, A, ep, e)
    ties, picks_made = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    print(nant, A, "ties", ties, "picks", picks_made)
    assert ties * 10 <= picks_made, (ties, picks_made)


def test_null_columns_and_a_teacher_are_the_taught_call():
    """frirl_hip_agent_begin_rows / _observe_rows with every column NULL and a teacher against frirl_hip_agent_begin_taught /
    _observe_taught on a twin batch, 30 steps of the point environment: the same bytes after every call."""
    import torch
    from tests.test_hip_external import PointEnv, assert_same, point_desc, state_arrays
    nant, A, E = 4, 5, 64
    d, env = point_desc(nant, A), PointEnv(nant - 1)
    rng = np.random.default_rng(9)
    ss = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    teacher = torch.from_numpy(np.where(rng.uniform(size=E) < 0.5, rng.integers(0, A, E), 32).astype(np.int32)).to(DEV)     # 32: the agent chooses
    pa, aa, ea = frirl_amd.fresh_batch(d, E, 512, DEV)
    pb, ab, eb = frirl_amd.fresh_batch(d, E, 512, DEV)
    rows = frirl_amd.HparamRows(E, DEV)
    act_a, _ = frirl_amd.agent_begin(pa, aa, ea, ss, teacher=teacher)
    act_b, _ = frirl_amd.agent_begin(pb, ab, eb, ss, teacher=teacher, rows=rows)
    assert_same(state_arrays(pa, ea), state_arrays(pb, eb), "begin")
    for t in range(30):
        oa, ra, sa = env.step(torch, ea.states, act_a)
        ob_, rb_, sb = env.step(torch, eb.states, act_b)
        na, _ = frirl_amd.agent_observe(pa, aa, ea, oa.contiguous(), ra.contiguous(), sa.to(torch.int32), teacher=teacher)
        nb, _ = frirl_amd.agent_observe(pb, ab, eb, ob_.contiguous(), rb_.contiguous(), sb.to(torch.int32), teacher=teacher, rows=rows)
        assert_same(state_arrays(pa, ea), state_arrays(pb, eb), t)
        act_a, act_b = torch.where(ea.done == 0, na, act_a), torch.where(eb.done == 0, nb, act_b)
    assert int(pa.nrules.max()) > 2 ** nant


# ---- 4. batch object and demo --------------------------------------------------------------------------------------------------------
def test_batch_object_trains_under_rows_and_reports_per_agent():
    """Nine mountaincar agents of a library-owned batch, agent e under set e mod 3, through frirl_hip_batch_set_hparams and
    frirl_hip_batch_train: frirl_hip_batch_agent_report gives every agent the episodes, rules, convergence flag and last episode of
    its set's oracle run.  While rows are set frirl_hip_batch_episode and _teach refuse (naming themselves) and a rejected
    frirl_hip_batch_set_hparams leaves them set; after clearing, frirl_hip_batch_episode runs again."""
    lib = frirl_amd.lib()
    env, E = "mountaincar", 9
    sets = rc.demo_sets(env)
    names = [sets[e % len(sets)] for e in range(E)]
    batch = frirl_amd.demo_batch_object(env, E, 512)
    try:
        frirl_amd.batch_set_hparams(batch, **rc.columns([hc.demo_desc(env, n) for n in names]))
        ran = C.c_int32(0)
        frirl_amd.check(lib.frirl_hip_batch_train(batch, hc.TRAJ_EPISODES[env], C.byref(ran)), "frirl_hip_batch_train")
        rep = frirl_amd.batch_agent_report(batch)
        for e, name in enumerate(names):
            r = hc.traj_run(env, name)
            fr = r["fr"]
            got = (int(rep["converged"][e]), int(rep["episodes"][e]), int(rep["rules"][e]), int(rep["ep_steps"][e]), float(rep["ep_reward"][e]))
            assert got == (r["converged"], r["episodes"], fr.five.R, fr.ep_steps, fr.ep_reward), (e, name, got)
        assert ran.value == max(hc.traj_run(env, n)["episodes"] for n in sets)
        st = frirl_amd.BatchStats()
        frirl_amd.check(lib.frirl_hip_batch_stats(batch, C.byref(st)), "frirl_hip_batch_stats")
        assert st.rules_sum == rep["rules"].sum() and st.total_env_steps == sum(hc.traj_run(env, n)["total_steps"] for n in names)
        assert lib.frirl_hip_batch_episode(batch) == -2 and b"frirl_hip_batch_episode" in lib.frirl_hip_last_error()
        res = frirl_amd.TeachResult()
        assert lib.frirl_hip_batch_teach(batch, 0, 1, None, 1, None, C.byref(res)) == -2 and b"frirl_hip_batch_teach" in lib.frirl_hip_last_error()
        with pytest.raises(frirl_amd.FrirlHipError, match="agent 4.*alpha"):
            frirl_amd.batch_set_hparams(batch, alpha=[0.5] * 4 + [float("nan")] + [0.5] * 4)
        assert lib.frirl_hip_batch_episode(batch) == -2, "a rejected set of rows must leave the batch as it was"
        frirl_amd.batch_set_hparams(batch)                      # clears
        assert lib.frirl_hip_batch_episode(batch) == 0
        assert (frirl_amd.batch_agent_report(batch)["episodes"] == rep["episodes"] + 1 - rep["converged"]).all()
    finally:
        lib.frirl_hip_batch_destroy(batch)


def test_demo_sweeps_three_sets_in_one_run(tmp_path):
    """frirl_demo --env mountaincar --agents 9 --max-episodes 14 --hparams f.txt: three `set` lines whose episode and rule means are the
    oracle's for that set (all three agents of a set are replicas)."""
    env = "mountaincar"
    sets = rc.demo_sets(env)
    f = tmp_path / "f.txt"
    f.write_text("# alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules\n" +
                 "".join(" ".join(repr(float(hc.demo_desc(env, n)[k])) for k in hc.HP_KEYS) + f"   # {n}\n" for n in sets))
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    r = subprocess.run([demo, "--env", env, "--agents", "9", "--max-episodes", str(hc.TRAJ_EPISODES[env]), "--hparams", str(f)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(f"hparams {env}: set ")]
    assert len(lines) == 3, r.stdout
    for s, (line, name) in enumerate(zip(lines, sets)):
        m = re.match(rf"hparams {env}: set (\d+) agents (\d+) converged (\d+) mean-episodes ([\d.]+) max-episodes (\d+) mean-rules ([\d.]+) mean-reward (-?[\d.]+)$", line)
        assert m, line
        ref = hc.traj_run(env, name)
        assert (int(m[1]), int(m[2]), int(m[3]), int(m[5])) == (s, 3, 3 * ref["converged"], ref["episodes"]), line
        assert float(m[4]) == ref["episodes"] and float(m[6]) == ref["fr"].five.R, (line, ref["episodes"], ref["fr"].five.R)
        assert abs(float(m[7]) - ref["fr"].ep_reward) <= 1e-6 * max(1.0, abs(ref["fr"].ep_reward)), line
