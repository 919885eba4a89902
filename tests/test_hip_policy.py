"""A trained rule base in the caller's environment, on the GPU: frirl_hip_policy_begin / _observe (one greedy step of Q caller-stepped
rows on ONE shared rule base) and the resumable reduction frirl_hip_reducer_* / reduce_external on top of them.

1. Stepped = in-kernel: a demo driven from outside (frirl_hip_env_step as the environment) gives the steps, reward and success of
   frirl_hip_rollout_shared and of the oracle, with and without exclude masks, identically for every lane-group shape.
2. The demos' reductions driven from outside equal frirl_hip_reduce_shared and the oracle's sequential loop.
3. Shapes no demo has (PointEnv, nant 2..8) against the pinned Python sequential loop of tests/test_policy_host.py.
4. Finished rows are skipped, reset masks, Q = 1 ... 65 536.
5. Misuse of the reducer returns EINVAL and leaves the rule base alone.
"""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests.test_hip_external import Mirror, PointEnv, generic_quantize, point_desc
from tests.test_hip_shared import shared_problem, start_states, trained
from tests.test_policy_host import SequentialReduction

pytestmark = pytest.mark.gpu
DEV = "cuda"


def group_shapes(A):
    """Every (lanes per row, rule slices) the launcher can choose for A actions (csrc/shape_ladder.h: lane_group / lane_slices with the options policy_group / policy_slices)."""
    G = 4 if A <= 4 else 8
    return [(1, 1), (G, 1), (G, 4), (G, 8)]


def drive_demo(prob, agent, env, s, masks=None, slot=None, shape=None, record=False):
    """Q greedy episodes of a demo stepped from outside: frirl_hip_env_step plays the caller's environment."""
    import torch
    Q = s.shape[0]
    old = None
    if shape is not None:
        old = (frirl_amd.set_option("policy_group", shape[0]), frirl_amd.set_option("policy_slices", shape[1]))
    try:
        rows = frirl_amd.PolicyRows(Q, DEV, exclude_mask=masks, rule_slot=slot)
        action, aidx = prob.policy_begin(agent, rows, s)
        trace = [aidx.clone()] if record else None
        states = s
        for t in range(agent.desc.max_steps):
            live = rows.done == 0
            obs, reward, success, q = frirl_amd.env_step(agent, action, states)
            nxt, nidx = prob.policy_observe(agent, rows, obs, reward, success, q_obs=q if env == "cartpole" else None)
            action = torch.where(live, nxt, action)
            states = obs
            if record:
                trace.append(torch.where(live, nidx, torch.full_like(nidx, -1)))
            if t % 25 == 24 and bool((rows.done != 0).all()):
                break
        torch.cuda.synchronize()
        assert bool((rows.done != 0).all())
        return rows, trace
    finally:
        if old is not None:
            frirl_amd.set_option("policy_group", old[0])
            frirl_amd.set_option("policy_slices", old[1])


# ---- 1. stepped = in-kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mountaincar", "cartpole", "acrobot"])
def test_stepped_rollout_equals_in_kernel_rollout(env, hip_option):
    import torch
    Q = 300
    fr = trained(env)
    prob, _ = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV)
    s_np = start_states(fr, Q, 5)
    s = torch.from_numpy(s_np).to(DEV)
    steps, reward, success, _ = prob.rollout_shared(agent, Q, start_states=s)
    hip_option("rollout_resident", 0)                      # the tiled in-kernel form: the same sums in the same order as the stepped form
    steps_t, reward_t, success_t, _ = prob.rollout_shared(agent, Q, start_states=s)
    torch.cuda.synchronize()
    traces = {}
    for shape in group_shapes(agent.A):
        rows, traces[shape] = drive_demo(prob, agent, env, s, shape=shape, record=True)
        assert torch.equal(rows.ep_steps, steps) and torch.equal(rows.ep_steps, steps_t), shape
        assert torch.equal(rows.success, success) and torch.equal(rows.success, success_t), shape
        assert torch.equal(rows.ep_reward.view(torch.int64), reward_t.view(torch.int64)), shape
        rel = ((rows.ep_reward - reward).abs() / reward.abs().clamp(min=1.0)).max().item()
        print(f"{env} shape {shape}: max relative reward difference to the default in-kernel form {rel:.3e}")
        assert rel <= 1e-9, shape
    first = traces[(1, 1)]
    for shape, tr in traces.items():
        assert len(tr) == len(first) and all(torch.equal(a, b) for a, b in zip(tr, first)), f"actions differ for shape {shape}"
    rows, _ = drive_demo(prob, agent, env, s)              # the shipped selection
    st, rw = rows.ep_steps.cpu().numpy(), rows.ep_reward.cpu().numpy()
    assert (st == steps.cpu().numpy()).all()
    for i in range(0, Q, 3 if env != "mountaincar" else 1):
        fr.set_start_state(s_np[i])
        fr.episode_eval()
        assert st[i] == fr.ep_steps, (i, st[i], fr.ep_steps)
        assert abs(rw[i] - fr.ep_reward) <= 1e-9 * max(1.0, abs(fr.ep_reward)), (i, rw[i], fr.ep_reward)


@pytest.mark.parametrize("env", ["mountaincar", "acrobot"])
def test_stepped_rollout_with_exclude_masks(env):
    """The twelve masks of tests/test_hip_shared.py::test_try_remove_masks_equal_compacted_rule_base."""
    import torch
    fr = trained(env)
    R = fr.five.R
    prob, maxR = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV)
    order = np.argsort(np.abs(fr.five.rconc[:R]), kind="stable")
    cand = [int(r) for r in order[-16:][::-1]] + [int(r) for r in order[:16]]
    slot = np.full(maxR, 255, dtype=np.uint8)
    for sl, r in enumerate(cand):
        slot[r] = sl
    masks = np.array([0, 1, 0x80000000, 0xffff, 0xffff0000, 0xffffffff, 0x00ff00ff, 0x0f0f0f0f, 0x3f, 0xfff, 0xffffff, 0xa5a5a5a5],
                     dtype=np.uint32).view(np.int32)
    masks_d, slot_d = torch.from_numpy(masks).to(DEV), torch.from_numpy(slot).to(DEV)
    Q = len(masks)
    steps, reward, success, _ = prob.rollout_shared(agent, Q, exclude_mask=masks_d, rule_slot=slot_d)
    torch.cuda.synchronize()
    s = torch.from_numpy(np.ascontiguousarray(np.tile(np.array(agent.desc.values_def[: fr.nstates]), (Q, 1)))).to(DEV)
    traces = {}
    for shape in group_shapes(agent.A):
        rows, traces[shape] = drive_demo(prob, agent, env, s, masks=masks_d, slot=slot_d, shape=shape, record=True)
        assert torch.equal(rows.ep_steps, steps) and torch.equal(rows.success, success), shape
        rel = ((rows.ep_reward - reward).abs() / reward.abs().clamp(min=1.0)).max().item()
        assert rel <= 1e-9, (shape, rel)
    first = traces[(1, 1)]
    for shape, tr in traces.items():
        assert len(tr) == len(first) and all(torch.equal(a, b) for a, b in zip(tr, first)), f"actions differ for shape {shape}"
    st, rw = steps.cpu().numpy(), reward.cpu().numpy()
    assert ((st != st[0]) | (rw != rw[0])).any(), "removals did not change the episode: the masks are not exercised"
    for i, m in enumerate(masks):
        fr2 = trained(env)
        for r in sorted([cand[sl] for sl in range(32) if (int(np.uint32(m)) >> sl) & 1], reverse=True):
            fr2.five.remove_rule(r)
        fr2.episode_eval()
        assert int(rows.ep_steps[i]) == fr2.ep_steps and abs(float(rows.ep_reward[i]) - fr2.ep_reward) <= 1e-9 * max(1.0, abs(fr2.ep_reward))


# ---- 2. the demos' reductions driven from outside --------------------------------------------------------------------------
def demo_copy(fr, rant0):
    import torch
    f = fr.five
    R0, nant = f.R, f.nant
    prob, maxR = shared_problem(fr, DEV)
    uidx = torch.zeros((1, nant, maxR), dtype=torch.int16, device=DEV)
    uidx[0, :, :R0] = torch.from_numpy(np.ascontiguousarray(f.uidx[:, :R0].astype(np.int16))).to(DEV)
    prob = frirl_amd.Problem(prob.u, prob.ve, prob.rb, prob.nrules, uidx)
    rant_d = torch.zeros((nant, maxR), dtype=torch.float64, device=DEV)
    rant_d[:, :R0] = torch.from_numpy(np.ascontiguousarray(rant0.T)).to(DEV)
    return prob, rant_d


@pytest.mark.parametrize("env,strategy", [("mountaincar", 1), ("mountaincar", 2), ("cartpole", 1), ("acrobot", 1)])
def test_external_reduction_of_the_demos(env, strategy):
    import torch
    fr = trained(env)
    f = fr.five
    R0, nant = f.R, f.nant
    rant0, rconc0, veval0 = np.array(f.rant[:R0]), np.array(f.rconc[:R0]), np.array(f.veval[:, :R0])
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV)
    start = torch.from_numpy(np.array(agent.desc.values_def[: nant - 1])).to(DEV)

    def step_fn(states, action):
        obs, reward, success, q = frirl_amd.env_step(agent, action, states)
        return (obs, reward, success, q) if env == "cartpole" else (obs, reward, success)

    results = {}
    for depth in ([0, 7, 1] if env == "mountaincar" else [0]):
        pa, rant_a = demo_copy(fr, rant0)
        pb, rant_b = demo_copy(fr, rant0)
        kept_a, res_a = frirl_amd.reduce_external(pa, agent, lambda Q: start.expand(Q, nant - 1).contiguous(), step_fn, strategy, 0.0, depth, rant=rant_a)
        kept_b, res_b = pb.reduce_shared(agent, strategy, 0.0, depth, rant=rant_b)
        torch.cuda.synchronize()
        assert (kept_a == kept_b).all() and res_a.rules_before == res_b.rules_before == R0
        for field in ("rules_after", "rounds", "rollouts", "steps_incremental"):
            assert getattr(res_a, field) == getattr(res_b, field), (depth, field)
        assert abs(res_a.reward - res_b.reward) <= 1e-9 * max(1.0, abs(res_b.reward))
        assert torch.equal(pa.rb.view(torch.int64), pb.rb.view(torch.int64)) and torch.equal(pa.nrules, pb.nrules)
        assert torch.equal(rant_a.view(torch.int64), rant_b.view(torch.int64)) and torch.equal(pa.uidx, pb.uidx)
        R1 = res_a.rules_after
        assert int(pa.nrules[0]) == R1 == len(kept_a)
        rb = pa.rb[0].cpu().numpy()
        assert (rb[:nant, :R1] == veval0[:, kept_a]).all() and (rb[nant, :R1] == rconc0[kept_a]).all() and (rb[:, R1:] == 0).all()
        assert (pa.uidx[0, :, :R1].cpu().numpy() == f.uidx[:, kept_a].astype(np.int16)).all() and bool((pa.uidx[0, :, R1:] == 0).all())
        results[depth] = (kept_a.copy(), res_a.rounds)
    fr.reduce(strategy, 0.0)                                         # the sequential loop (mutates the oracle's rule base)
    R1 = f.R
    kept0, rounds0 = results[0]
    assert len(kept0) == R1 and 0 < R1 < R0
    assert (np.array(f.rant[:R1]) == rant0[kept0]).all() and (np.array(f.rconc[:R1]) == rconc0[kept0]).all()
    assert rounds0 == -(-R0 // 10)
    for depth, (k, rounds) in results.items():
        assert len(k) == R1 and (k == kept0).all(), depth


# ---- 3. a shape no demo has -------------------------------------------------------------------------------------------------
def train_point_agent(d, nant, start, maxR=1024, episodes=30):
    """One agent of the caller's environment through agent_begin / agent_observe until its rule base is complete or `episodes`."""
    import torch
    env = PointEnv(nant - 1)
    prob, agent, envs = frirl_amd.fresh_batch(d, 1, maxR, DEV)
    conv = frirl_amd.Convergence(prob, DEV)
    ss = torch.from_numpy(start[None].copy()).to(DEV)
    for ep in range(episodes):
        action, _ = frirl_amd.agent_begin(prob, agent, envs, ss)
        for t in range(d["max_steps"]):
            live = envs.done == 0
            obs, reward, success = env.step(torch, envs.states, action)
            nxt, _ = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32))
            action = torch.where(live, nxt, action)
        conv.update(prob, agent, envs)
        if int(conv.converged[0]) == 1:
            break
    torch.cuda.synchronize()
    return prob, agent, envs


def external_reduction_with_trace(prob, agent, env, start_d, strategy, rant):
    """reduce_external's round loop written out, keeping every row's action index of every step (for the tie rule of the checker)."""
    import torch
    red = frirl_amd.Reducer(prob, agent, strategy, 0.0, 0, rant)
    rounds = []
    try:
        while red.next_round() > 0:
            states = start_d.expand(red.Q, start_d.numel()).contiguous()
            action, aidx = red.begin(states)
            picks = [aidx.clone()]
            live = red.Q
            while live > 0:
                obs, reward, success = env.step(torch, states, action)
                states = obs.contiguous()
                action, aidx, live = red.observe(states, reward.contiguous(), success.to(torch.int32))
                picks.append(aidx.clone())
            red.end_round()
            rounds.append(torch.stack(picks).cpu().numpy())
        return red.result() + (rounds,)
    finally:
        red.close()


def test_external_reduction_of_new_shapes_follows_the_sequential_loop():
    import torch
    clean_shapes = 0
    report = []
    for nant, A in ((2, 3), (4, 5), (6, 11), (8, 3)):
        d = point_desc(nant, A)
        env = PointEnv(nant - 1)
        start = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, nant - 1))
        trained_prob, agent, envs = train_point_agent(d, nant, start)
        R0 = int(trained_prob.nrules[0])
        rant0 = envs.rant[0, :, :R0].cpu().numpy().T.copy()
        rconc0 = trained_prob.rb[0, nant, :R0].cpu().numpy().copy()
        veval0 = trained_prob.rb[0, :nant, :R0].cpu().numpy().copy()
        start_d = torch.from_numpy(start).to(DEV)

        def env_fn(states, action):
            x, r, ok = env.step(np, states[None], np.array([action]))
            return x[0], float(r[0]), int(ok[0]), generic_quantize(d, x[0])

        shape_ties = 0
        for strategy in (1, 2):
            prob = frirl_amd.Problem(trained_prob.u, trained_prob.ve, trained_prob.rb.clone(), trained_prob.nrules.clone(), trained_prob.uidx.clone())
            rant_d = envs.rant[0].clone()
            kept, res, rounds = external_reduction_with_trace(prob, agent, env, start_d, strategy, rant_d)
            torch.cuda.synchronize()

            def device_pick(i, bits, step):
                tr = rounds[0] if i < 0 else rounds[1 + i // 10]
                lane = 0 if i < 0 else (1 << (i % 10)) - 1 + bits
                return int(tr[step, lane]) if step < tr.shape[0] else None

            args = (d["u"], d["ve"], rant0, rconc0, d["action_ve"], d["grids"][nant - 1], start, env_fn, d["max_steps"], d["reward_good_above"])
            alone = SequentialReduction(*args)                          # the oracle on its own: are there ties at all?
            kept_alone = alone.run(strategy)
            seq = SequentialReduction(*args, device_pick=device_pick)   # ties within 1e-12 relative follow the device
            kept_seq = seq.run(strategy)
            report.append((nant, A, strategy, R0, len(kept_seq), alone.near_ties, seq.ties, kept_alone == kept_seq))
            print("shape nant=%d A=%d strategy=%d: %d -> %d rules, oracle-only near ties %d, device-followed ties %d, oracle-only keeps the same rules: %s" % report[-1])
            shape_ties += alone.near_ties
            assert list(kept) == kept_seq, (nant, A, strategy)
            assert res.rules_before == R0 and res.rules_after == len(kept_seq) == int(prob.nrules[0])
            assert res.steps_incremental == seq.steps_incremental and res.rounds == -(-R0 // 10)
            assert 1 <= res.rules_after < R0, "the case must remove at least one rule and keep at least one"
            R1 = res.rules_after
            rb = prob.rb[0].cpu().numpy()
            assert (rb[:nant, :R1] == veval0[:, kept]).all() and (rb[nant, :R1] == rconc0[kept]).all() and (rb[:, R1:] == 0).all()
            assert (rant_d[:, :R1].cpu().numpy() == rant0[kept].T).all() and bool((rant_d[:, R1:] == 0).all())
        clean_shapes += shape_ties == 0
    assert clean_shapes >= 3, report


# ---- 3b. a Shepard power other than nant --------------------------------------------------------------------------------------
def oracle_trained_point_base(nant, A, p, episodes=30):
    """A rule base of the caller's environment learned by the oracle alone at Shepard power p (no GPU needed): description, environment,
    start state, oracle rule base."""
    d = point_desc(nant, A)
    env = PointEnv(nant - 1)
    start = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, nant - 1))
    m = Mirror(d, start, 1024, p=p)
    for _ in range(episodes):
        m.episode(env, None)
        if m.converged:
            break
    return d, env, start, m.five


def sequential_reduction_at_power(nant, A, p, strategy, device_pick=None):
    d, env, start, f = oracle_trained_point_base(nant, A, p)
    R0 = f.R

    def env_fn(states, action):
        x, r, ok = env.step(np, states[None], np.array([action]))
        return x[0], float(r[0]), int(ok[0]), generic_quantize(d, x[0])

    seq = SequentialReduction(d["u"], d["ve"], np.array(f.rant[:R0]), np.array(f.rconc[:R0]), d["action_ve"], d["grids"][nant - 1], start, env_fn,
                              d["max_steps"], d["reward_good_above"], device_pick=device_pick, p=p)
    return d, env, start, f, seq, seq.run(strategy)


@pytest.mark.parametrize("nant,A", [(3, 3), (5, 11)])
def test_external_reduction_at_power_2_follows_the_sequential_loop(nant, A):
    """frirl_hip_reducer_* with agent.p = 2 (the policy kernels' run-time-power variants) on a rule base the oracle learned at p = 2, with
    policy_group forced to 1 and to 4 / 8, against SequentialReduction(p=2).  Picks that follow the device inside a 1e-12 tie of the
    oracle: at most 10 % (the oracle alone has such near-ties at 0 of 512 picks for nant 3 / A 3 and 0 of 5266 for nant 5 / A 11, which the test asserts too)."""
    import torch
    p, strategy = 2, 1
    d, env, start, f, alone, kept_alone = sequential_reduction_at_power(nant, A, p, strategy)
    assert alone.near_ties * 10 <= alone.picks
    R0 = f.R
    rb = torch.from_numpy(f.device_layout(R0 + 8 + (R0 & 1))[None].copy()).to(DEV)
    agent = frirl_amd.demo_agent(d, DEV, p=p)
    start_d = torch.from_numpy(start).to(DEV)
    u, ve = torch.from_numpy(d["u"]).to(DEV), torch.from_numpy(d["ve"]).to(DEV)
    for group in (1, 4 if A <= 4 else 8):
        prob = frirl_amd.Problem(u, ve, rb.clone(), torch.tensor([R0], dtype=torch.int32, device=DEV))
        old = frirl_amd.set_option("policy_group", group)
        try:
            kept, res, rounds = external_reduction_with_trace(prob, agent, env, start_d, strategy, None)
            torch.cuda.synchronize()
        finally:
            frirl_amd.set_option("policy_group", old)

        def device_pick(i, bits, step):
            tr = rounds[0] if i < 0 else rounds[1 + i // 10]
            lane = 0 if i < 0 else (1 << (i % 10)) - 1 + bits
            return int(tr[step, lane]) if step < tr.shape[0] else None

        _, _, _, _, seq, kept_seq = sequential_reduction_at_power(nant, A, p, strategy, device_pick=device_pick)
        assert seq.ties * 10 <= seq.picks, (seq.ties, seq.picks)
        assert list(kept) == kept_seq, (nant, A, group)
        assert res.rules_before == R0 and res.rules_after == len(kept_seq) == int(prob.nrules[0])
        assert res.steps_incremental == seq.steps_incremental and res.rounds == -(-R0 // 10)
        assert 1 <= res.rules_after < R0, "the case must remove at least one rule and keep at least one"
        R1 = res.rules_after
        got = prob.rb[0].cpu().numpy()
        assert (got[:nant, :R1] == np.array(f.veval[:, :R0])[:, kept]).all() and (got[nant, :R1] == np.array(f.rconc[:R0])[kept]).all()
        assert (got[:, R1:] == 0).all()


def test_stepped_rollout_with_exclude_masks_at_power_2():
    """The twelve masks of test_stepped_rollout_with_exclude_masks at agent.p = 2 on a mountaincar rule base the oracle learned at p = 2:
    the stepped roll-out equals the in-kernel one and the oracle's greedy episode on the COMPACTED rule base, for policy_group 1 and 4
    and policy_slices 1, 4 and 8.  With p != nant the launcher ignores policy_slices (the variants without rule slices run), so slices = 8
    must give the actions of slices = 1 step by step."""
    import torch
    env = "mountaincar"

    def learned():
        fr = ob.Frirl(env, trig_mode=1)
        fr.set_power(2)
        fr.run(max_episodes=13)
        return fr

    fr = learned()
    R = fr.five.R
    prob, maxR = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV, p=2)
    order = np.argsort(np.abs(fr.five.rconc[:R]), kind="stable")
    cand = [int(r) for r in order[-16:][::-1]] + [int(r) for r in order[:16]]
    slot = np.full(maxR, 255, dtype=np.uint8)
    for sl, r in enumerate(cand):
        slot[r] = sl
    masks = np.array([0, 1, 0x80000000, 0xffff, 0xffff0000, 0xffffffff, 0x00ff00ff, 0x0f0f0f0f, 0x3f, 0xfff, 0xffffff, 0xa5a5a5a5],
                     dtype=np.uint32).view(np.int32)
    masks_d, slot_d = torch.from_numpy(masks).to(DEV), torch.from_numpy(slot).to(DEV)
    Q = len(masks)
    steps, reward, success, _ = prob.rollout_shared(agent, Q, exclude_mask=masks_d, rule_slot=slot_d)
    torch.cuda.synchronize()
    s = torch.from_numpy(np.ascontiguousarray(np.tile(np.array(agent.desc.values_def[: fr.nstates]), (Q, 1)))).to(DEV)
    traces = {}
    for shape in group_shapes(agent.A):
        rows, traces[shape] = drive_demo(prob, agent, env, s, masks=masks_d, slot=slot_d, shape=shape, record=True)
        assert torch.equal(rows.ep_steps, steps) and torch.equal(rows.success, success), shape
        rel = ((rows.ep_reward - reward).abs() / reward.abs().clamp(min=1.0)).max().item()
        assert rel <= 1e-9, (shape, rel)
    first = traces[(1, 1)]
    for shape, tr in traces.items():
        assert len(tr) == len(first) and all(torch.equal(a, b) for a, b in zip(tr, first)), f"actions differ for shape {shape}"
    st, rw = steps.cpu().numpy(), reward.cpu().numpy()
    assert ((st != st[0]) | (rw != rw[0])).any(), "removals did not change the episode: the masks are not exercised"
    for i, m in enumerate(masks):
        fr2 = learned()
        for r in sorted([cand[sl] for sl in range(32) if (int(np.uint32(m)) >> sl) & 1], reverse=True):
            fr2.five.remove_rule(r)
        fr2.episode_eval()
        assert int(st[i]) == fr2.ep_steps and abs(float(rw[i]) - fr2.ep_reward) <= 1e-9 * max(1.0, abs(fr2.ep_reward)), (i, st[i], fr2.ep_steps)


# ---- 4. masks and skipping ---------------------------------------------------------------------------------------------------
def test_finished_rows_are_skipped_and_reset_restarts_selected_rows():
    import torch
    env = "mountaincar"
    fr = trained(env)
    prob, _ = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV)
    Q = 200
    s = torch.from_numpy(start_states(fr, Q, 9)).to(DEV)
    rows = frirl_amd.PolicyRows(Q, DEV)
    action, _ = prob.policy_begin(agent, rows, s)
    states = s
    for t in range(40):
        obs, reward, success, q = frirl_amd.env_step(agent, action, states)
        action, _ = prob.policy_observe(agent, rows, obs, reward, success)
        states = obs
    # finish half of the rows by hand: the next call must not touch them
    done_mask = torch.arange(Q, device=DEV) % 2 == 0
    rows.done[done_mask] = 1
    before = dict(steps=rows.ep_steps.clone(), reward=rows.ep_reward.clone(), success=rows.success.clone())
    obs, reward, success, q = frirl_amd.env_step(agent, action, states)
    io, out, out_idx = frirl_amd._agent_io(prob, obs, None, reward, success, E=Q)
    out.fill_(float("nan"))
    out_idx.fill_(-5)
    frirl_amd.check(frirl_amd.lib().frirl_hip_policy_observe(C.byref(prob.tables), C.byref(prob._bases), C.byref(agent.desc), C.byref(rows.desc),
                                                             C.byref(io), frirl_amd._stream()), "frirl_hip_policy_observe")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[done_mask]).all()) and bool((out_idx[done_mask] == -5).all())
    assert not bool(torch.isnan(out[~done_mask]).any()) and bool((out_idx[~done_mask] >= 0).all())
    assert torch.equal(rows.ep_steps[done_mask], before["steps"][done_mask]) and torch.equal(rows.ep_steps[~done_mask], before["steps"][~done_mask] + 1)
    assert torch.equal(rows.ep_reward[done_mask], before["reward"][done_mask]) and torch.equal(rows.success[done_mask], before["success"][done_mask])
    # a reset mask restarts only the selected rows
    snap = dict(done=rows.done.clone(), steps=rows.ep_steps.clone(), reward=rows.ep_reward.clone())
    reset = torch.arange(Q, device=DEV) % 3 == 0
    act2, idx2 = prob.policy_begin(agent, rows, s, reset=reset.to(torch.uint8))
    fresh = frirl_amd.PolicyRows(Q, DEV)
    act3, idx3 = prob.policy_begin(agent, fresh, s)
    torch.cuda.synchronize()
    assert bool((rows.ep_steps[reset] == 0).all()) and bool((rows.done[reset] == 0).all()) and bool((rows.ep_reward[reset] == 0).all())
    assert torch.equal(rows.ep_steps[~reset], snap["steps"][~reset]) and torch.equal(rows.done[~reset], snap["done"][~reset])
    assert torch.equal(rows.ep_reward[~reset], snap["reward"][~reset])
    assert torch.equal(act2[reset], act3[reset]) and torch.equal(idx2[reset], idx3[reset])


@pytest.mark.parametrize("Q", [1, 255, 257, 65536])
def test_first_action_agrees_with_get_best_action_shared(Q):
    import torch
    fr = trained("acrobot")
    assert fr.five.R == 367
    prob, _ = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe("acrobot"), DEV)
    s = torch.from_numpy(start_states(fr, Q, 21)).to(DEV)
    _, best = prob.get_best_action_shared(s, agent.action_ve)
    for shape in [None] + group_shapes(agent.A):
        old = None
        if shape is not None:
            old = (frirl_amd.set_option("policy_group", shape[0]), frirl_amd.set_option("policy_slices", shape[1]))
        try:
            rows = frirl_amd.PolicyRows(Q, DEV)
            action, aidx = prob.policy_begin(agent, rows, s)
            # one observed step, so that the observe path runs at this size too
            obs, reward, success, q = frirl_amd.env_step(agent, action, s)
            nxt, nidx = prob.policy_observe(agent, rows, obs, reward, success)
            _, best2 = prob.get_best_action_shared(q, agent.action_ve)
            torch.cuda.synchronize()
        finally:
            if old is not None:
                frirl_amd.set_option("policy_group", old[0])
                frirl_amd.set_option("policy_slices", old[1])
        assert torch.equal(aidx, best), shape
        assert torch.equal(action, agent.grid_values[prob.nant - 1][best.long()])
        assert torch.equal(nidx, best2), shape
        assert bool((rows.ep_steps == 1).all())


# ---- 5. misuse ------------------------------------------------------------------------------------------------------------------
def test_reducer_calls_out_of_order_are_refused():
    import torch
    env = "mountaincar"
    fr = trained(env)
    prob, _ = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV)
    ns = fr.nstates
    start = torch.from_numpy(np.array(agent.desc.values_def[:ns])).to(DEV)
    L = frirl_amd.lib()
    snapshot = (prob.rb.clone(), prob.nrules.clone())

    def unchanged():
        torch.cuda.synchronize()
        return torch.equal(prob.rb.view(torch.int64), snapshot[0].view(torch.int64)) and torch.equal(prob.nrules, snapshot[1])

    red = frirl_amd.Reducer(prob, agent, 1)
    try:
        obs1 = start.expand(1, ns).contiguous()
        io, _, _ = frirl_amd._agent_io(prob, obs1, E=1)
        assert L.frirl_hip_reducer_begin(red.h, C.byref(io)) == -2            # begin before next_round
        assert L.frirl_hip_reducer_end_round(red.h) == -2
        assert red.next_round() == 1
        q = C.c_int32()
        assert L.frirl_hip_reducer_next_round(red.h, C.byref(q)) == -2        # next_round inside a round
        action, _ = red.begin(obs1)
        assert L.frirl_hip_reducer_begin(red.h, C.byref(io)) == -2            # begin twice
        assert L.frirl_hip_reducer_end_round(red.h) == -2 and b"have not ended" in L.frirl_hip_last_error()   # the row is live
        assert unchanged()
        states, live = obs1, 1
        while live > 0:
            obs, reward, success, _ = frirl_amd.env_step(agent, action, states)
            action, _, live = red.observe(obs, reward, success)
            states = obs
        red.end_round()
        # first try-remove round: closing it with live rows is refused and nothing is compacted
        Q = red.next_round()
        assert Q == 1023
        states = start.expand(Q, ns).contiguous()
        action, _ = red.begin(states)
        obs, reward, success, _ = frirl_amd.env_step(agent, action, states)
        action, _, live = red.observe(obs, reward, success)
        assert live > 0
        assert L.frirl_hip_reducer_end_round(red.h) == -2 and unchanged()
        while live > 0:
            states = obs
            obs, reward, success, _ = frirl_amd.env_step(agent, action, states)
            action, _, live = red.observe(obs, reward, success)
        red.end_round()
        # run the rest, then observe after the last round
        def step_rest():
            while red.next_round() > 0:
                st = start.expand(red.Q, ns).contiguous()
                act, _ = red.begin(st)
                lv = red.Q
                while lv > 0:
                    o, r, sc, _ = frirl_amd.env_step(agent, act, st)
                    act, _, lv = red.observe(o, r, sc)
                    st = o
                red.end_round()
        step_rest()
        kept, res = red.result()
        final = (prob.rb.clone(), prob.nrules.clone())
        io2, _, _ = frirl_amd._agent_io(prob, obs, None, reward, success, E=obs.shape[0])
        assert L.frirl_hip_reducer_observe(red.h, C.byref(io2), None) == -2   # observe after the last round
        assert L.frirl_hip_reducer_begin(red.h, C.byref(io)) == -2
        assert red.next_round() == 0
        torch.cuda.synchronize()
        assert torch.equal(prob.rb.view(torch.int64), final[0].view(torch.int64)) and torch.equal(prob.nrules, final[1])
    finally:
        red.close()
    # and the result is the reduction
    fr.reduce(1, 0.0)
    assert res.rules_after == fr.five.R == len(kept) and res.rules_after < res.rules_before
