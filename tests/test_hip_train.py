"""Batched construct runs on the GPU (frirl_sequential_run's loop for E agents: episode_begin / episode_steps /
convergence_update) against the oracle's whole demo run with the portable trig.

Every agent starts from the reference's initial 2^nant corner rule base and must end exactly where the oracle ends:
same number of episodes, same rule count, same antecedents in the same order (bit-exact), consequents within the
1e-6 contract (asserted at 1e-9)."""
import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("env,episodes,steps,rules", [("mountaincar", 29, 15548, 110), ("cartpole", 58, 33002, 182), ("acrobot", 110, 21207, 367)])
def test_batched_training_reaches_the_oracle_rule_base(env, episodes, steps, rules):
    import torch
    E = 6
    dev = torch.device("cuda", 0)
    fr = ob.Frirl(env, trig_mode=1)
    assert fr.run() == 1 and fr.five.R == rules and fr.total_steps == steps       # the portable trig learns the same rule base size
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 1024, dev)
    total = torch.zeros((E,), dtype=torch.int64, device=dev)

    def on_episode(ep, conv):
        total.add_(envs.ep_steps.long() * (conv.episodes == ep).long())

    conv = frirl_amd.train(prob, agent, envs, on_episode=on_episode)
    torch.cuda.synchronize()
    assert (conv.converged == 1).all()
    assert (conv.episodes == episodes).all(), conv.episodes.tolist()
    assert (total == steps).all(), total.tolist()
    assert (prob.nrules == rules).all()
    f = fr.five
    rant = envs.rant[:, :, :rules].cpu().numpy()
    assert (rant == f.rant[:rules].T[None]).all(), "antecedents / rule order"
    q = prob.rb[:, prob.nant, :rules].cpu().numpy()
    rel = np.abs(q - f.rconc[None, :rules]) / np.maximum(np.abs(f.rconc[None, :rules]), 1e-9)
    assert rel.max() <= 1e-9, rel.max()


def test_epsilon_greedy_streams():
    """Exploration (frirl_e_greedy_selection.c:28-33, batched with a counter-based per-environment stream):
    epsilon = 0 or no_random = 1 reproduce the greedy run; a seed reproduces itself; trajectories are keyed by the
    GLOBAL environment id (independent of how the batch is sharded); the exploration rate is about epsilon."""
    import torch
    dev = torch.device("cuda", 0)
    K = 120

    def run(E, **kw):
        prob, agent, envs = frirl_amd.demo_fresh_batch("acrobot", E, 512, dev, **kw)
        frirl_amd.episode_begin(prob, agent, envs)
        acts = []
        for _ in range(K):
            frirl_amd.episode_steps(prob, agent, envs, 1)
            acts.append(envs.q_ant[:, prob.nant - 1].clone())
        torch.cuda.synchronize()
        return torch.stack(acts, 1), envs.states.clone(), prob.nrules.clone()

    g_act, g_states, g_rules = run(8)
    a0, s0, r0 = run(8, epsilon=0.0, no_random=0, seed=7)
    assert (a0 == g_act).all() and (s0 == g_states).all()
    a1, s1, r1 = run(8, epsilon=0.3, no_random=1, seed=7)
    assert (a1 == g_act).all()
    x_act, x_states, x_rules = run(8, epsilon=0.3, no_random=0, seed=7)
    y_act, y_states, _ = run(8, epsilon=0.3, no_random=0, seed=7)
    assert (x_act == y_act).all() and (x_states == y_states).all(), "same seed, same trajectory"
    z_act, _, _ = run(8, epsilon=0.3, no_random=0, seed=8)
    assert not (z_act == x_act).all()
    assert not (x_act[0] == x_act[1]).all(), "environments have different streams"
    # sharding invariance: environments 4..7 of the 8-batch == a 4-batch whose env_id_base is 4
    h_act, h_states, _ = run(4, epsilon=0.3, no_random=0, seed=7, env_id_base=4)
    assert (h_act == x_act[4:]).all() and (h_states == x_states[4:]).all()
    # exploration rate: a random pick differs from the greedy pick 2/3 of the time (3 actions, clamped round() is not
    # uniform: P = 1/6, 1/3, 1/2), so the observed deviation rate from a greedy replay is below epsilon; just bound it
    dev_rate = (x_act != g_act).double().mean().item()
    assert 0.02 < dev_rate < 0.6


@pytest.mark.parametrize("env", ["mountaincar", "cartpole", "acrobot"])
def test_evaluation_mode_rollout(env):
    """policy roll-out without updates (frirl_test_run / reduction replays: reduction_state = 1,
    frirl_episode.c:155).  Train on the device, then evaluate: the rule bases stay bit-identical and the greedy
    episode equals the oracle's roll-out on its own trained rule base (steps and reward exactly)."""
    import torch
    dev = torch.device("cuda", 0)
    E = 4
    fr = ob.Frirl(env, trig_mode=1)
    assert fr.run() == 1
    fr.episode_eval()
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 1024, dev)
    conv = frirl_amd.train(prob, agent, envs)
    assert (conv.converged == 1).all()
    before = prob.rb.clone()
    nr = prob.nrules.clone()
    d = frirl_amd.demo_describe(env)
    ev_agent = frirl_amd.demo_agent(d, dev, evaluate=1)
    frirl_amd.episode_begin(prob, ev_agent, envs)
    frirl_amd.episode_steps(prob, ev_agent, envs, ev_agent.desc.max_steps)
    torch.cuda.synchronize()
    assert (prob.rb == before).all() and (prob.nrules == nr).all(), "evaluation must not touch the rule bases"
    assert (envs.ep_steps == fr.ep_steps).all(), (envs.ep_steps.tolist(), fr.ep_steps)
    assert (envs.ep_reward == fr.ep_reward).all()


@pytest.mark.parametrize("env", ["mountaincar", "acrobot"])
def test_persistent_episode_kernel_is_bit_identical_to_step_kernel(env):
    """frirl_hip_episode_run (rule base, tables and episode state resident in LDS, many steps per launch) must give
    exactly the bits of the same number of frirl_hip_episode_step launches -- including environments that outgrow the
    LDS slab (status FULL, continued by the step kernel)."""
    import torch
    dev = torch.device("cuda", 0)
    E = 64

    def run(persistent, lds_rules=256):
        prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 1024, dev)
        for ep in range(5):
            frirl_amd.episode_begin(prob, agent, envs)
            if persistent:
                frirl_amd.episode_run(prob, agent, envs, agent.desc.max_steps, lds_rules)
                torch.cuda.synchronize()
                if not bool((envs.done != 0).all()):              # slab full somewhere: finish with the step kernel
                    assert (envs.status[envs.done == 0] == frirl_amd.UPD_FULL).all()
                    frirl_amd.episode_steps(prob, agent, envs, agent.desc.max_steps)
            else:
                frirl_amd.episode_steps(prob, agent, envs, agent.desc.max_steps)
            torch.cuda.synchronize()
            assert (envs.done == 1).all()
        return [prob.rb.clone(), prob.nrules.clone(), envs.states.clone(), envs.q_ant.clone(), envs.ep_steps.clone(), envs.ep_reward.clone(),
                envs.fus.clone(), envs.rant.clone(), prob.uidx.clone()]       # uidx: the 16-bit mirror must follow LDS appends too

    ref = run(False)
    for lds in (256, 1024):
        got = run(True, lds)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert (a == b).all(), (lds, i)
    assert int(ref[1].max()) > 32
    if env == "acrobot":
        # force the overflow path: a 256-rule slab is too small once acrobot's rule base grows past it
        prob, agent, envs = frirl_amd.demo_fresh_batch(env, 4, 1024, dev)
        conv = frirl_amd.train(prob, agent, envs, max_episodes=60, persistent_max_rules=1024, lanes=False)
        prob2, agent2, envs2 = frirl_amd.demo_fresh_batch(env, 4, 1024, dev)
        conv2 = frirl_amd.train(prob2, agent2, envs2, max_episodes=60, persistent=False, lanes=False)
        torch.cuda.synchronize()
        assert (prob.rb == prob2.rb).all() and (prob.nrules == prob2.nrules).all() and int(prob.nrules.max()) > 256
        assert (prob.uidx == prob2.uidx).all()


@pytest.mark.parametrize("env", ["mountaincar", "acrobot"])
def test_persistent_episode_kernel_keeps_the_index_mirror_in_sync(env):
    """frirl_hip_episode_run appends rules in LDS; the 16-bit universe-index mirror (frirl_hip_rulebases.uidx ==
    FIVERB.rseqant_uindex, five_add_rule.c:76) must follow: afterwards uidx equals the oracle's indices and the
    compressed rule-distance scan gives the bits of the f64 scan."""
    import os
    import torch
    dev = torch.device("cuda", 0)
    E = 8
    fr = ob.Frirl(env, trig_mode=1)
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 1024, dev)
    for _ in range(4):
        fr.episode()
        frirl_amd.episode_begin(prob, agent, envs)
        frirl_amd.episode_run(prob, agent, envs, agent.desc.max_steps, 1024)
        torch.cuda.synchronize()
        assert (envs.done == 1).all()
    R = fr.five.R
    assert (prob.nrules == R).all() and R > 2 ** prob.nant
    got = prob.uidx[:, :, :R].cpu().numpy().astype(np.int64)
    assert (got == fr.five.uidx[None, :, :R]).all(), "uidx mirror out of sync after LDS appends"
    # rb[e][k][r] == ve[k][uidx[e][k][r]]
    ve = prob.ve.cpu().numpy()
    rb = prob.rb[:, : prob.nant, :R].cpu().numpy()
    assert (rb == ve[np.arange(prob.nant)[None, :, None], got]).all()
    x = envs.q_ant.clone()
    d_idx, h_idx = prob.rule_distance(x)
    plain = frirl_amd.Problem(prob.u, prob.ve, prob.rb, prob.nrules)          # no mirror: the f64 columns are streamed
    d_f64, h_f64 = plain.rule_distance(x)
    torch.cuda.synchronize()
    assert (h_idx == h_f64).all() and (d_idx[:, :R].view(torch.int64) == d_f64[:, :R].view(torch.int64)).all()


def test_non_default_shepard_power():
    """A Shepard power p != nant (the reference accepts any p, FIVEInit.c:89-93): the LDS-persistent episode kernel (with its hand-off
    to the step kernel when the slab fills: status FULL) must give exactly the bits of the plain step kernel, and the lane-group
    kernel's run-time-power variants must learn the same rule bases."""
    import torch
    dev = torch.device("cuda", 0)

    def run(persistent):
        prob, agent, envs = frirl_amd.demo_fresh_batch("acrobot", 5, 1024, dev, p=2)
        assert agent.desc.p == 2
        conv = frirl_amd.train(prob, agent, envs, max_episodes=40, persistent=persistent, persistent_max_rules=1024, lanes=False)
        torch.cuda.synchronize()
        return prob, envs, conv

    pa, ea, ca = run(True)
    pb, eb, cb = run(False)
    assert (pa.rb == pb.rb).all() and (pa.nrules == pb.nrules).all() and (pa.uidx == pb.uidx).all()
    assert (ea.rant == eb.rant).all() and (ca.episodes == cb.episodes).all()
    assert int(pa.nrules.max()) > 64, "the rule bases grew"
    # the lane-group kernel (run-time power variants) learns the same rule bases: decisions exact, Q to rounding
    pl, agent_l, el = frirl_amd.demo_fresh_batch("acrobot", 5, 1024, dev, p=2)
    cl = frirl_amd.train(pl, agent_l, el, max_episodes=40, lanes=True)
    torch.cuda.synchronize()
    assert (pl.nrules == pb.nrules).all() and (cl.episodes == cb.episodes).all()
    assert (el.rant == eb.rant).all() and (pl.rb[:, : pl.nant] == pb.rb[:, : pb.nant]).all()
    qa, qb = pl.rb[:, pl.nant], pb.rb[:, pb.nant]
    assert ((qa - qb).abs() <= 1e-9 * qb.abs().clamp_min(1e-9)).all()
    # ... and differs from the default power (the option is really used)
    pd, agent_d, ed = frirl_amd.demo_fresh_batch("acrobot", 5, 1024, dev)
    frirl_amd.train(pd, agent_d, ed, max_episodes=40, lanes=True)
    torch.cuda.synchronize()
    assert not (pd.rb[:, pd.nant] == qa).all()


def test_rollout_on_shared_rule_base_with_non_default_power():
    """frirl_hip_rollout_shared with p != nant (run-time power variants) == the per-environment step kernels in evaluate mode."""
    import torch
    dev = torch.device("cuda", 0)
    prob, agent, envs = frirl_amd.demo_fresh_batch("mountaincar", 1, 512, dev, p=2)
    frirl_amd.train(prob, agent, envs, max_episodes=12, lanes=False)
    Q = 300
    d = frirl_amd.demo_describe("mountaincar")
    g = torch.Generator(device=dev).manual_seed(3)
    lo = torch.tensor([d["grids"][k].min() for k in range(2)], dtype=torch.float64, device=dev)
    hi = torch.tensor([d["grids"][k].max() for k in range(2)], dtype=torch.float64, device=dev)
    ss = (lo + (hi - lo) * torch.rand((Q, 2), dtype=torch.float64, device=dev, generator=g)).contiguous()
    one = frirl_amd.Problem(prob.u, prob.ve, prob.rb[0:1].clone(), prob.nrules[0:1].clone())
    steps, reward, _, _ = one.rollout_shared(agent, Q, start_states=ss)
    # reference: Q copies of the rule base, evaluate-mode episodes through the step kernel
    many = frirl_amd.Problem(prob.u, prob.ve, prob.rb[0:1].expand(Q, -1, -1).contiguous(), prob.nrules[0:1].expand(Q).contiguous())
    ev_agent = frirl_amd.demo_agent(d, dev, p=2, evaluate=1)
    envs2 = frirl_amd.Envs(many, dev, keep_rant=False, start_states=ss)
    frirl_amd.episode_begin(many, ev_agent, envs2)
    frirl_amd.episode_steps(many, ev_agent, envs2, ev_agent.desc.max_steps)
    torch.cuda.synchronize()
    same = (steps == envs2.ep_steps)
    assert same.float().mean() > 0.98, same.float().mean()        # sequential vs tree sums: a near-tie may flip an action
    assert ((reward - envs2.ep_reward).abs()[same] <= 1e-9 * envs2.ep_reward.abs()[same].clamp_min(1.0)).all()


# ---- p = 2 against the oracle (the two tests above compare kernels with kernels) ---------------------------------------------------
@pytest.mark.parametrize("kernel", ["fused_step", "lane_group"])
def test_power_2_learning_follows_the_oracle(kernel):
    """Three mountaincar episodes at agent.p = 2 through the fused step kernel and through the lane-group learner (their variants
    without rule slices), every environment followed by the oracle with its rule base's power set to 2 (portable trig on both sides):
    steps, rewards, rule counts and appended antecedents exact, learned Q within 1e-6."""
    import numpy as np
    import torch
    from oracle import binding as ob
    dev = torch.device("cuda", 0)
    fr = ob.Frirl("mountaincar", trig_mode=1)
    fr.set_power(2)
    E = 4
    prob, agent, envs = frirl_amd.demo_fresh_batch("mountaincar", E, 512, dev, p=2)
    assert agent.desc.p == 2 and fr.five.c.p == 2
    for _ in range(3):
        fr.episode()
        frirl_amd.episode_begin(prob, agent, envs)
        if kernel == "fused_step":
            frirl_amd.episode_steps(prob, agent, envs, agent.desc.max_steps)
        else:
            frirl_amd.episode_run_lanes(prob, agent, envs, agent.desc.max_steps)
        torch.cuda.synchronize()
        assert (envs.done.cpu().numpy() == 1).all()
        assert (envs.ep_steps.cpu().numpy() == fr.ep_steps).all() and (envs.ep_reward.cpu().numpy() == fr.ep_reward).all()
        R = fr.five.R
        assert (prob.nrules.cpu().numpy() == R).all()
        assert (envs.rant[:, :, :R].cpu().numpy() == fr.five.rant[:R].T[None]).all(), "appended rule antecedents"
        q, ref = prob.rb[:, prob.nant, :R].cpu().numpy(), np.array(fr.five.rconc[:R])
        assert (np.abs(q - ref[None]) <= 1e-6 * np.maximum(np.abs(ref[None]), 1e-9)).all()
    assert fr.five.R > 2 ** prob.nant, "rules were inserted"
    other = ob.Frirl("mountaincar", trig_mode=1)          # the default power learns something else: p is really used by the oracle
    for _ in range(3):
        other.episode()
    assert other.five.R != fr.five.R or (np.array(other.five.rconc[: fr.five.R]) != np.array(fr.five.rconc[: fr.five.R])).any()


def test_power_2_rollouts_on_a_shared_rule_base_follow_the_oracle():
    """frirl_hip_rollout_shared at agent.p = 2 (the shared roll-out's variants without rule slices, resident and tiled) on a rule base
    the oracle learned at p = 2, against the oracle's greedy episode from the same start states: steps exact, reward 1e-9."""
    import numpy as np
    import torch
    from oracle import binding as ob
    from tests.test_hip_shared import shared_problem, start_states
    dev = torch.device("cuda", 0)
    fr = ob.Frirl("mountaincar", trig_mode=1)
    fr.set_power(2)
    fr.run(max_episodes=13)
    assert fr.five.R > 40
    prob, _ = shared_problem(fr, dev)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe("mountaincar"), dev, p=2)
    Q = 70                                                         # two workgroups, the second one ragged
    s = start_states(fr, Q, 5)
    outs = []
    for resident in (1, 0):
        old = frirl_amd.set_option("rollout_resident", resident)
        try:
            steps, reward, success, _ = prob.rollout_shared(agent, Q, start_states=torch.from_numpy(s).to(dev))
            torch.cuda.synchronize()
        finally:
            frirl_amd.set_option("rollout_resident", old)
        outs.append((steps.cpu().numpy(), reward.cpu().numpy()))
    for steps, reward in outs:
        for i in range(Q):
            fr.set_start_state(s[i])
            fr.episode_eval()
            assert steps[i] == fr.ep_steps, (i, steps[i], fr.ep_steps)
            assert abs(reward[i] - fr.ep_reward) <= 1e-9 * max(1.0, abs(fr.ep_reward)), (i, reward[i], fr.ep_reward)
    assert len(set(outs[0][0].tolist())) > 3, "the start states lead to different episodes"
