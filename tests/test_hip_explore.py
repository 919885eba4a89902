"""Epsilon-greedy exploration (no_random == 0, epsilon > 0) on every device path against an independent reference.

1. The stream and the pick themselves (frirl_hip_explore_check: rng_unit / e_greedy of csrc/envs.h as the kernels call them) against
   tests/explore_ref.py: units bit for bit, actions exactly, at the key edges.
2. Whole exploring episodes of the three demos against the oracle (oracle/frirl_oracle.c restates the stream and its keys): E
   environments that start identically and differ through their streams only -- the fused step kernel step by step; the
   multi-step, LDS-persistent and lane-group forms at episode boundaries; the persistent learner at the end of its construct loop.
3. Exploring roll-outs on a shared trained rule base: the tiled lane form with and without try-remove masks, the resident forms
   (stage kernel with parked rows, one wave per row, wave pair) and the caller-stepped policy API in every lane-group shape, all
   against the oracle's roll-out per row: steps, reward bits, success, final-state bits.

tests/test_explore_ref.py shows on the CPU that the cases have exploring picks that change the action and no near-tie at a greedy pick,
so nothing here allows for ties.  The new shapes (nant 2..8, A 3 / 11) explore in tests/test_hip_external.py."""
import itertools

import numpy as np
import pytest

import frirl_amd
from tests import explore_cases as xc
from tests import explore_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-9)


# ---- 1. the probe ----------------------------------------------------------------------------------------------------------
def probe_keys(A):
    """(row, episode, step, greedy) tuples: the key edges crossed with each other, then rows 0..N-1 at ordinary keys; > 4096 in all."""
    rows = [0, 1, 2, 3, 4, 5, 8, 77, 1000, 2 ** 31, 2 ** 32 - 1]
    keys = [(r, ep, st) for r, ep, st in itertools.product(rows, [0, 1, 2 ** 31 - 1], [0, 1, 999, 2 ** 24])]
    keys += [(i, 1 + i % 3, i // 3) for i in range(4096)]
    return [(r, ep, st, (r + ep + st) % A) for r, ep, st in keys]


@pytest.mark.parametrize("env_id_base", [0, 77, 2 ** 32 - 3, 2 ** 40])
@pytest.mark.parametrize("A", [1, 2, 3, 21, 32])
def test_stream_and_pick_match_the_reference(A, env_id_base):
    import torch
    d = frirl_amd.demo_describe("mountaincar")
    seed = 0x1234567890ABCDEF
    keys = probe_keys(A)
    env = torch.tensor([k[0] for k in keys], dtype=torch.int64, device=DEV)
    ep = torch.tensor([k[1] for k in keys], dtype=torch.int64, device=DEV)
    st = torch.tensor([k[2] for k in keys], dtype=torch.int64, device=DEV)
    greedy = torch.tensor([k[3] for k in keys], dtype=torch.int32, device=DEV)
    gids = [env_id_base + k[0] for k in keys]
    if env_id_base == 2 ** 32 - 3:
        assert min(gids) < 2 ** 32 <= max(gids), "rows on both sides of 2^32"
    want_units = np.array([[er.unit(seed, g, k[1], k[2], 0), er.unit(seed, g, k[1], k[2], 1)] for g, k in zip(gids, keys)])
    if A > 1:       # the inputs are not vacuous: by the reference alone every action is drawn and the clamp is taken
        drawn = [er.random_action(A, seed, g, k[1], k[2]) for g, k in zip(gids, keys)]
        assert {a for a, _ in drawn} == set(range(A)), "every action 0..A-1 is drawn"
        assert sum(c for _, c in drawn) >= 1, "round(u * A) == A occurs"
    for epsilon, no_random in itertools.product([0.0, 2.0 ** -53, 0.3, 1.0, 1.5], [0, 1]):
        agent = frirl_amd.demo_agent(d, DEV, epsilon=epsilon, no_random=no_random, seed=seed, env_id_base=env_id_base)
        agent.desc.A = A                                   # the probe reads A, epsilon, no_random, seed and env_id_base only
        action, units = frirl_amd.explore_check(agent, env, ep, st, greedy)
        torch.cuda.synchronize()
        assert (units.cpu().numpy().view(np.uint64) == want_units.view(np.uint64)).all(), (epsilon, no_random)
        want = np.array([er.pick(k[3], A, epsilon, no_random, seed, g, k[1], k[2]) for g, k in zip(gids, keys)])
        got = action.cpu().numpy()
        assert (got == want).all(), (epsilon, no_random, int((got != want).sum()))
        if no_random == 0 and epsilon >= 1.0:              # a unit never exceeds 1.0: every pick explores
            assert (want == np.array([a for a, _ in [er.random_action(A, seed, g, k[1], k[2]) for g, k in zip(gids, keys)]])).all()
        if no_random == 1 or epsilon == 0.0:
            assert (want == np.array([k[3] for k in keys])).all()


# ---- 2. whole exploring episodes against the oracle -------------------------------------------------------------------------
def fresh(env, **kw):
    return frirl_amd.demo_fresh_batch(env, xc.E, xc.MAXR, DEV, max_steps=xc.MAX_STEPS, epsilon=xc.EPSILON, no_random=0, seed=xc.SEEDS[env],
                                      env_id_base=xc.BASE, **kw)


def check_episode_end(prob, envs, row, where):
    """Steps, reward, final state, rule count, antecedents and flag exact; consequents to 1e-9 (as test_fused_episode_steps_follow_oracle)."""
    nant = prob.nant
    assert (envs.done.cpu().numpy() == 1).all(), where
    steps, reward = envs.ep_steps.cpu().numpy(), envs.ep_reward.cpu().numpy()
    nrules, rb, rant = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), envs.rant.cpu().numpy()
    states, fus = envs.states.cpu().numpy(), envs.fus.cpu().numpy()
    for e, r in enumerate(row):
        end = r["end"]
        R = end["R"]
        assert steps[e] == end["steps"] and reward[e] == end["reward"], (where, e, steps[e], end["steps"])
        assert (states[e].view(np.uint64) == end["states"].view(np.uint64)).all(), (where, e)
        assert nrules[e] == R, (where, e, nrules[e], R)
        assert (rant[e, :, :R] == end["rant"].T).all() and (rb[e, :nant, :R] == end["veval"]).all(), (where, e)
        assert rel(rb[e, nant, :R], end["rconc"]).max() <= 1e-9, (where, e)
        assert fus[e] == end["fus"], (where, e)


@pytest.mark.parametrize("env", xc.DEMOS)
def test_step_kernel_follows_the_exploring_oracle(env):
    """frirl_hip_episode_begin + frirl_hip_episode_step, every step: the continuous state bit for bit, the quantised state and the
    chosen action (its value, bit for bit: the action grids have distinct values), the rule count before the step and whether the
    update appended a rule."""
    import torch
    episodes, _ = xc.learning_case(env)
    prob, agent, envs = fresh(env)
    nant = prob.nant
    for ep, row in enumerate(episodes):
        frirl_amd.episode_begin(prob, agent, envs)
        torch.cuda.synchronize()
        assert (envs.episode.cpu().numpy() == ep + 1).all()
        first = envs.q_ant.cpu().numpy()[:, nant - 1]
        assert (first == np.array([r["first"] for r in row])).all(), (ep, "first action (un-quantised start state)")
        for t in range(max(len(r["trace"]) for r in row)):
            live = [e for e, r in enumerate(row) if t < len(r["trace"])]
            before = prob.nrules.cpu().numpy()
            frirl_amd.episode_step(prob, agent, envs)
            torch.cuda.synchronize()
            st, qa, after, status = envs.states.cpu().numpy(), envs.q_ant.cpu().numpy(), prob.nrules.cpu().numpy(), envs.status.cpu().numpy()
            for e in live:
                _, cur_states, cur_q, R_before = row[e]["trace"][t]
                R_after = row[e]["trace"][t + 1][3] if t + 1 < len(row[e]["trace"]) else row[e]["end"]["R"]
                assert before[e] == R_before and after[e] == R_after, (ep, t, e)
                assert (st[e].view(np.uint64) == cur_states.view(np.uint64)).all(), (ep, t, e)
                assert (qa[e].view(np.uint64) == cur_q.view(np.uint64)).all(), (ep, t, e, qa[e], cur_q)
                assert (status[e] == frirl_amd.UPD_INSERTED) == (R_after > R_before), (ep, t, e, status[e])
                assert status[e] in (frirl_amd.UPD_EXACT, frirl_amd.UPD_SPREAD, frirl_amd.UPD_INSERTED, frirl_amd.UPD_SKIPPED)
        check_episode_end(prob, envs, row, (env, ep))


LDS_SLAB = 256          # rules per environment of frirl_hip_episode_run's LDS slab in the "persistent" form
# frirl_hip_episode_run serves up to 8 actions and tables of up to 16 KiB (frirl_amd.can_run_persistent): not cartpole, whose episodes
# the step kernel runs ("steps7")
MULTI_STEP_FORMS = [(env, form) for env in xc.DEMOS for form in ("steps7", "persistent", "lanes") if not (env == "cartpole" and form == "persistent")]


@pytest.mark.parametrize("env,form", MULTI_STEP_FORMS)
def test_multi_step_forms_follow_the_exploring_oracle(env, form):
    """frirl_hip_episode_steps(7), frirl_hip_episode_run (rule bases resident in LDS; the shapes it serves) and the lane-group
    learner frirl_hip_episode_run_lanes, compared at the end of every episode."""
    import torch
    episodes, _ = xc.learning_case(env)
    prob, agent, envs = fresh(env)
    if form == "persistent":
        assert frirl_amd.can_run_persistent(prob, agent)
        # a rule base that outgrows the slab comes back not done (status FULL): by the oracle alone these cases stay inside it, with
        # the margin of 128 rules that frirl_amd.train keeps when it chooses a slab
        assert max(r["end"]["R"] for row in episodes for r in row) + 128 <= LDS_SLAB
    for ep, row in enumerate(episodes):
        frirl_amd.episode_begin(prob, agent, envs)
        if form == "steps7":
            for _ in range(-(-xc.MAX_STEPS // 7)):
                frirl_amd.episode_steps(prob, agent, envs, 7)
        elif form == "persistent":
            frirl_amd.episode_run(prob, agent, envs, xc.MAX_STEPS, LDS_SLAB)
        else:
            frirl_amd.episode_run_lanes(prob, agent, envs, xc.MAX_STEPS)
        torch.cuda.synchronize()
        check_episode_end(prob, envs, row, (env, form, ep))


@pytest.mark.parametrize("slices", [1, 8])
@pytest.mark.parametrize("env", xc.DEMOS)
def test_persistent_learner_follows_the_exploring_oracle(env, slices, hip_option):
    """frirl_hip_learn_train with one lane and with 8 lanes per agent, launches of 50 steps' work (every launch boundary falls inside an
    episode of up to 120 steps, so the episode key is carried from launch to launch), against the oracle's construct loop on the same
    streams: episodes, convergence, steps and the rule base per agent."""
    import torch
    want = xc.construct_case(env)
    hip_option("learn_slices", slices)
    prob, agent, envs = fresh(env)
    assert frirl_amd.learn_supported(prob, agent)
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=xc.EPISODES + 1, budget=50)
    torch.cuda.synchronize()
    assert run.launches >= 3
    converged, eps, total = run.conv.converged.cpu().numpy(), run.conv.episodes.cpu().numpy(), run.steps_total.cpu().numpy()
    stream_pos = envs.episode.cpu().numpy()
    nant = prob.nant
    nrules, rb, rant, uidx = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), envs.rant.cpu().numpy(), prob.uidx.cpu().numpy().astype(np.int64) & 0xFFFF
    for e, w in enumerate(want):
        end = w["end"]
        R = end["R"]
        assert converged[e] == w["converged"] and stream_pos[e] == w["episodes"], (e, converged[e], stream_pos[e], w["episodes"])
        assert eps[e] == w["episodes"], (e, eps[e], w["episodes"])
        assert total[e] == w["total_steps"], (e, total[e], w["total_steps"])
        assert nrules[e] == R, (e, nrules[e], R)
        assert (rant[e, :, :R] == end["rant"].T).all() and (rb[e, :nant, :R] == end["veval"]).all() and (uidx[e, :, :R] == end["uidx"]).all(), e
        assert rel(rb[e, nant, :R], end["rconc"]).max() <= 1e-9, e


# ---- 3. exploring roll-outs on a shared rule base ---------------------------------------------------------------------------
def shared_setup(env, masked):
    import torch
    from tests.test_hip_shared import shared_problem
    case = xc.rollout_case(env, masked)
    fr = xc.trained(env)
    assert fr.five.R == case["R"]
    prob, maxR = shared_problem(fr, DEV)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), DEV, max_steps=xc.ROLLOUT_MAX_STEPS, epsilon=xc.EPSILON, no_random=0,
                                 seed=xc.SEEDS[env], env_id_base=xc.BASE)
    masks = slot = None
    if masked:
        sl = np.full(maxR, 255, dtype=np.uint8)
        for i, r in enumerate(case["cand"]):
            sl[r] = i
        m = np.array([xc.MASKS[q % 4] for q in range(xc.Q)], dtype=np.uint32).view(np.int32)
        masks, slot = torch.from_numpy(m).to(DEV), torch.from_numpy(sl).to(DEV)
    return case, prob, agent, torch.from_numpy(case["starts"]).to(DEV), masks, slot


def check_rows(case, steps, reward, success, final, where):
    steps, reward, success = steps.cpu().numpy(), reward.cpu().numpy(), success.cpu().numpy()
    assert (steps == case["steps"]).all(), (where, np.flatnonzero(steps != case["steps"])[:8], steps[:8], case["steps"][:8])
    assert (reward.view(np.uint64) == case["reward"].view(np.uint64)).all(), where
    assert (success == case["success"]).all(), where
    if final is not None:
        assert (final.cpu().numpy().view(np.uint64) == case["final"].view(np.uint64)).all(), where


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("env", xc.DEMOS)
def test_tiled_rollouts_follow_the_exploring_oracle(env, masked, hip_option):
    """The lane form of csrc/shared.hip (frirl_hip_rollout_shared with the resident form switched off), one lane and a lane group per
    row, with and without try-remove masks."""
    import torch
    case, prob, agent, s, masks, slot = shared_setup(env, masked)
    hip_option("rollout_resident", 0)
    for group in (1, 4 if agent.A <= 4 else 8):
        hip_option("rollout_group", group)
        steps, reward, success, final = prob.rollout_shared(agent, xc.Q, start_states=s, exclude_mask=masks, rule_slot=slot)
        torch.cuda.synchronize()
        check_rows(case, steps, reward, success, final, (env, masked, group))


@pytest.mark.parametrize("form", ["default", "staged", "one_wave", "pair"])
@pytest.mark.parametrize("env", xc.DEMOS)
def test_resident_rollouts_follow_the_exploring_oracle(env, form, hip_option):
    """The LDS-resident forms of csrc/rollout.hip: as shipped for 64 rows; "staged": the stage kernel with 4 lanes per row parks every
    row that outlives ROLLOUT_CAP steps and a later stage finishes them; "one_wave" / "pair": a whole wave per row without and with
    the speculative stepper (3 actions; with 21 actions both select the 16-lane stage kernel)."""
    import torch
    case, prob, agent, s, _, _ = shared_setup(env, False)
    assert frirl_amd.lib().frirl_hip_rollout_resident_rules(prob.nant, agent.A, 0, agent.desc.env_kind) >= case["R"]
    if form == "staged":
        assert int((case["steps"] > xc.ROLLOUT_CAP).sum()) >= 8, "by the reference alone, rows are parked"
        hip_option("rollout_slices", 4)
        hip_option("rollout_cap", xc.ROLLOUT_CAP)
    elif form == "one_wave":
        hip_option("rollout_pair", 0)
    elif form == "pair":
        hip_option("rollout_pair", 1)
    steps, reward, success, final = prob.rollout_shared(agent, xc.Q, start_states=s)
    torch.cuda.synchronize()
    check_rows(case, steps, reward, success, final, (env, form))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("env", xc.DEMOS)
def test_stepped_policy_follows_the_exploring_oracle(env, masked, hip_option):
    """frirl_hip_policy_begin / _observe with frirl_hip_env_step as the caller's environment, in every lane-group shape the launcher
    can choose: the keys of the in-kernel roll-outs, checked against the oracle.  The rows' state lives in the caller's environment:
    the final state of a row is the observation of the step at which the row turned done."""
    import torch
    from tests.test_hip_policy import group_shapes
    case, prob, agent, s, masks, slot = shared_setup(env, masked)
    for shape in group_shapes(agent.A):
        hip_option("policy_group", shape[0])
        hip_option("policy_slices", shape[1])
        rows = frirl_amd.PolicyRows(xc.Q, DEV, exclude_mask=masks, rule_slot=slot)
        action, _ = prob.policy_begin(agent, rows, s)
        states, final = s, torch.full_like(s, float("nan"))
        for t in range(xc.ROLLOUT_MAX_STEPS):
            live = rows.done == 0
            obs, reward, success, q = frirl_amd.env_step(agent, action, states)
            nxt, _ = prob.policy_observe(agent, rows, obs, reward, success, q_obs=q if env == "cartpole" else None)
            ended = live & (rows.done != 0)
            final = torch.where(ended[:, None], obs, final)
            action = torch.where(live, nxt, action)
            states = obs
        torch.cuda.synchronize()
        assert bool((rows.done != 0).all())
        check_rows(case, rows.ep_steps, rows.ep_reward, rows.success, final, (env, masked, shape))
