"""The learning kernels off the demos' hyper-parameters (alpha, gamma, the qdiff bounds, weight_significant, skip_rules), against the
oracle, whose own treatment of them is pinned to the genuine reference by tests/test_hparams_ref.py.  The sets, the cases and the
conditions under which a case means something (sensitivity, branch counts, margins of the greedy picks, near-tie caps) are in
tests/hparams_cases.py and asserted on the CPU by tests/test_hparams_ref.py; the measured figures are in that module's docstrings.

Bars: rule counts, branch taken, sticky flag, appended antecedents / VE columns / index mirror, episode steps, reward bits: exact.
Consequents: <= 1e-9 relative (the contract is 1e-6).
"""
import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import hparams_cases as hc
from tests.problems import Batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
assert (hc.EXACT, hc.SPREAD, hc.INSERTED, hc.SKIPPED) == (frirl_amd.UPD_EXACT, frirl_amd.UPD_SPREAD, frirl_amd.UPD_INSERTED, frirl_amd.UPD_SKIPPED)
TOL = 1e-9            # consequents, every test of this module


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-9)


# ---- update level: frirl_hip_update_sarsa, no arg-max -----------------------------------------------------------------------------
# launch form: E, index mirror, device maxR (the mirror is only read above 2048 rules of capacity)
FORMS = {"e96_1024": (96, False, None), "e256_idx": (256, True, 2304), "e256_f64": (256, False, None)}


def update_problem(c, compressed, maxR):
    t, E = c.table, c.E
    b = Batch.__new__(Batch)
    b.nant, b.U, b.E, b.A, b.maxR = t.nant, t.U, E, t.A, maxR or c.maxR
    b.u, b.ve = t.u, t.ve
    b.nrules = np.full(E, t.R, dtype=np.int32)
    b.rb = np.zeros((E, t.nant + 1, b.maxR))
    b.rb[:, : t.nant, : t.R] = t.veval
    b.rb[:, t.nant, : t.R] = t.rconc
    b.uidx = np.zeros((E, t.nant, b.maxR), dtype=np.uint32)
    b.uidx[:, :, : t.R] = t.uidx
    return b.to_device(DEV, compressed=compressed)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(hc.SETS))
@pytest.mark.parametrize("table", range(len(hc.UPDATE_TABLES)), ids=hc.UPDATE_TABLE_IDS)
def test_update_sarsa_over_the_sets(table, name, form):
    """Six random rounds and the two crafted ones of hparams_cases.UpdateCase through each launch form of frirl_hip_update_sarsa (1024
    threads below 256 environments; 256 threads with and without the 16-bit index mirror), every environment against its own oracle
    rule base after every round.  Round A queries the rule an environment has just inserted with qdiff inside the bounds: SKIPPED and
    nothing changed under skip_rules = 1, an EXACT update under skip_rules = 0; round B with qdiff outside: the flag is cleared and the
    rule updated.  Over the case every branch is seen; SKIPPED exactly when skip_rules = 1."""
    import torch
    E, compressed, maxR = FORMS[form]
    c = hc.update_case(table, name, E)
    t, nant, h = c.table, c.table.nant, c.h
    prob = update_problem(c, compressed, maxR)
    assert (prob.uidx is not None) == compressed
    kind = t.source.env if isinstance(t.source, ob.Frirl) else frirl_amd.ENV_EXTERNAL
    agent = frirl_amd.Agent(DEV, nant, t.grids, t.grid_div, np.zeros(nant), t.action_ve, h["alpha"], h["gamma"], h["qdiff_pos"], h["qdiff_neg"],
                            h["weight_thr"], h["skip_rules"], 0, kind)
    rant0 = torch.zeros((E, nant, prob.maxR), dtype=torch.float64, device=DEV)
    rant0[:, :, : t.R] = dev(np.ascontiguousarray(t.rant.T))[None]
    envs = frirl_amd.Envs(prob, DEV, rant_init=rant0)
    envs.fus.copy_(dev(c.fus0))
    seen = set()
    q_prev = prob.rb[:, nant, : t.R + 16].cpu().numpy()
    for rnd, r in enumerate(c.rounds):
        frirl_amd.update_sarsa(prob, agent, envs, dev(r["q_ant"]), dev(r["reward"]), dev(r["cur"]), active=dev(r["active"]))
        torch.cuda.synchronize()
        top = int(r["R"].max())
        nr, st, fus_d = prob.nrules.cpu().numpy(), envs.status.cpu().numpy(), envs.fus.cpu().numpy()
        rb, rant = prob.rb[:, :, :top].cpu().numpy(), envs.rant[:, :, :top].cpu().numpy()
        uidx = prob.uidx[:, :, :top].cpu().numpy().astype(np.int64) & 0xFFFF if compressed else None
        assert (nr == r["R"]).all(), (rnd, np.nonzero(nr != r["R"])[0][:8])
        for e in range(E):
            n = int(r["R"][e])
            if not r["active"][e]:
                assert st[e] == frirl_amd.UPD_INACTIVE
                continue
            want = r["status"][e]
            assert st[e] == want, (rnd, e, st[e], want)
            assert fus_d[e] == r["fus"][e], (rnd, e, want)
            if want == hc.INSERTED:
                ra, ve, ui = r["new_rule"][e]
                assert (rant[e, :, n - 1] == ra).all(), "appended rule antecedents (grid-snapped)"
                assert (rb[e, :nant, n - 1] == ve).all(), "appended VE column"
                if compressed:
                    assert (uidx[e, :, n - 1] == ui).all(), "appended index-mirror column"
            if want == hc.SKIPPED:
                assert (rb[e, nant, :n].view(np.uint64) == q_prev[e, :n].view(np.uint64)).all(), (rnd, e, "a skipped update wrote")
            if r["crafted"][e]:
                inside = rnd == hc.ROUNDS or h["qdiff_pos"] >= 1e29
                assert want == (hc.SKIPPED if inside and h["skip_rules"] == 1 else hc.EXACT), (rnd, e, want)
            assert rel(rb[e, nant, :n], r["rconc"][e]).max() <= TOL, (rnd, e, want)
            seen.add(want)
        q_prev = np.zeros((E, top + 16))
        q_prev[:, :top] = rb[:, nant]
        if rnd >= hc.ROUNDS:
            assert r["crafted"].sum() >= E // 8, "the crafted rounds need environments with the flag set"
    need = {hc.EXACT, hc.SPREAD} | ({hc.INSERTED} if name != "never_insert" else set())
    assert need <= seen, seen
    assert (hc.SKIPPED in seen) == (h["skip_rules"] == 1), seen
    if name == "never_insert":
        assert hc.INSERTED not in seen and (prob.nrules == t.R).all()


def lane_counts(weights, thr, block):
    """Per environment the most rules with weight > thr that one lane of a `block`-thread pair sweep holds (rules r with
    r % (2 * block) in {2l, 2l + 1}), and the number of such rules; NaN rows (exact hits) count nothing."""
    import torch
    q = (weights > thr)
    E, maxR = q.shape
    lane = (torch.arange(maxR, device=q.device) % (2 * block)) // 2
    per = torch.zeros((E, block), dtype=torch.int64, device=q.device).index_add_(1, lane, q.long())
    return per.max(1).values, q.sum(1)


@pytest.mark.parametrize("name", ["thr_small", "thr_big"])
@pytest.mark.parametrize("env,E,R", [("acrobot", 40, 1500), ("acrobot", 40, 3000), ("mountaincar", 64, 3000), ("cartpole", 64, 5000)])
def test_spread_candidates_equal_the_second_sweep_at_other_thresholds(env, E, R, name, hip_option):
    """tests/test_hip_sarsa.py::test_spread_candidates_equal_the_second_sweep (with its near-duplicate rules planted in one lane's slots)
    at weight_significant 0.002 and 0.3: the write-back from the candidates tracked in the Q(s,a) sweep (two per lane, fall-back to
    the sweep on a third) gives the bits of the forced second sweep (agent.debug_flags bit 0), and other bits than a run at the
    default 0.05.  Only the acrobot kernels track candidates (episode_kernel.h: 4 antecedents or more, at most 4 actions): one wave per
    environment at a capacity of 1756 rules, 256 threads at 3256; mountaincar and cartpole run their second sweep either way and are
    here for the threshold alone.  Counted from the device's own Shepard weights at the points the six steps update: at 0.002 some
    lane of the acrobot sweep that runs holds three or more qualifying rules (the fall-back); at 0.3 no environment has more than
    three in all."""
    import torch
    dev0 = torch.device("cuda", 0)
    hip_option("step_track", 1)
    thr = hc.overrides(name, {})["weight_thr"]
    outs = []
    lane64 = lane256 = total = 0
    for flags, w in ((0, thr), (1, thr), (0, 0.05)):
        prob, agent, envs = frirl_amd.demo_batch(env, E, R, R + 256, dev0, seed=13)
        agent.desc.debug_flags = flags
        agent.desc.weight_significant = w
        nant = prob.nant
        d = frirl_amd.demo_describe(env)
        for e in range(8):          # rules 10, 11, 138, 139, 522, 523: near-duplicates of one point next to the start state
            for j, r in enumerate((10, 11, 138, 139, 522, 523)):
                for k in range(nant):
                    base_idx = int(np.argmin(np.abs(d["u"][k] - (d["values_def"][k] if k < nant - 1 else d["grids"][k][0]))))
                    idx = min(max(base_idx + (1 if (k == (j % (nant - 1))) else 0) + (1 if k == 0 else 0), 0), prob.U - 1)
                    prob.uidx[e, k, r] = idx
                    prob.rb[e, k, r] = prob.ve[k, idx]
                    envs.rant[e, k, r] = prob.u[k, idx]
                prob.rb[e, nant, r] = 100.0 + j
        frirl_amd.episode_begin(prob, agent, envs)
        seen = torch.zeros(6, dtype=torch.int64, device=dev0)
        for _ in range(6):
            if flags == 0 and w == thr:
                wts, _ = prob.vag_concl_weight(envs.q_ant.contiguous())
                l64, n = lane_counts(wts, thr, 64)
                l256, _ = lane_counts(wts, thr, 256)
                lane64, lane256, total = max(lane64, int(l64.max())), max(lane256, int(l256.max())), max(total, int(n.max()))
            frirl_amd.episode_steps(prob, agent, envs, 1)
            seen += torch.bincount(envs.status.long(), minlength=6)
        torch.cuda.synchronize()
        outs.append((prob.rb.clone(), prob.nrules.clone(), envs.states.clone(), envs.q_ant.clone(), envs.fus.clone(), seen))
    for i, (a, b) in enumerate(zip(outs[0][:5], outs[1][:5])):
        assert (a == b).all(), i
    assert (outs[0][5] == outs[1][5]).all() and int(outs[0][5][frirl_amd.UPD_SPREAD]) > 0, outs[0][5].tolist()
    assert not (outs[0][0] == outs[2][0]).all(), "the threshold changes nothing: the same consequents as at 0.05"
    print(env, name, "most qualifying rules per lane (64 / 256 threads)", lane64, lane256, "per environment", total)
    if name == "thr_small":
        if env == "acrobot":
            assert (lane64 if R + 256 <= 2048 else lane256) >= 3, (lane64, lane256)
    else:
        assert total <= 3, total          # weights sum to 1


# ---- trajectories: every kernel with its own copy of the update --------------------------------------------------------------------
def check_trajectory(r, prob, envs, total, E):
    """Every agent of a batch of replicas against the oracle's run r (hparams_cases.traj_run)."""
    from tests.test_hip_learn import check_agent_against_oracle
    fr = r["fr"]
    assert (total.cpu().numpy() == r["total_steps"]).all(), (total.tolist(), r["total_steps"])
    assert (envs.ep_steps.cpu().numpy() == fr.ep_steps).all() and (envs.ep_reward.cpu().numpy() == fr.ep_reward).all(), "last episode: steps, reward bits"
    assert (envs.fus.cpu().numpy() == int(fr.fus)).all()
    for e in sorted({0, E // 2, E - 1}):
        check_agent_against_oracle(fr, prob, envs, e)


@pytest.mark.parametrize("kernel", ["fused_step", "lane_group"])
@pytest.mark.parametrize("env,name", hc.TRAJ_CASES)
def test_construct_run_follows_the_oracle(env, name, kernel):
    """The admitted cases (greedy picks inside the kernel, the oracle's own margin >= 1e-6) through frirl_amd.train without the
    LDS-persistent kernel: once the per-step kernels (episode_kernel.h), once frirl_hip_episode_run_lanes (lanes.hip); 5 replicas."""
    import torch
    E = 5
    dev0 = torch.device("cuda", 0)
    r = hc.traj_run(env, name)
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, name), E, hc.TRAJ_MAXR, dev0)
    total = torch.zeros((E,), dtype=torch.int64, device=dev0)

    def on_episode(ep, conv):
        total.add_(envs.ep_steps.long() * (conv.episodes == ep).long())

    conv = frirl_amd.train(prob, agent, envs, max_episodes=hc.TRAJ_EPISODES[env], on_episode=on_episode, persistent=False, lanes=kernel == "lane_group")
    torch.cuda.synchronize()
    assert (conv.converged == r["converged"]).all() and (conv.episodes == r["episodes"]).all(), conv.episodes.tolist()
    check_trajectory(r, prob, envs, total, E)


LEARN_CASES = [(env, name, slices, 700) for env, name in hc.TRAJ_CASES for slices in (0, 1, 64)] + \
              [("cartpole", "thr_small", 0, 5), ("acrobot", "thr0", 0, 5)]


@pytest.mark.parametrize("env,name,slices,budget", LEARN_CASES)
def test_persistent_learner_follows_the_oracle(env, name, slices, budget, hip_option):
    """The admitted cases through frirl_hip_learn_train (learn_kernel.h: flags against a carried lower bound of the Shepard sum, at most
    8 flagged rules per lane, walk of everything otherwise), 21 replicas, for the default lane-group size and 1 and 64 rule slices.
    With a budget of 5 steps every launch starts with the bound unknown.  Under thr0 the extra rule visits in run.work[:, 1] must
    cover a walk of every rule in every spread (see below); under thr_small they are only required to be there, which the snapped-point
    sweeps alone can satisfy: when a walk is forced there depends on the lanes per agent the launch plan picks, which a test cannot
    fix below the kernel's minimum for the shape."""
    import torch
    E = 21
    dev0 = torch.device("cuda", 0)
    if slices:
        hip_option("learn_slices", slices)
    r = hc.traj_run(env, name)
    prob, agent, envs = frirl_amd.fresh_batch(hc.demo_desc(env, name), E, hc.TRAJ_MAXR, dev0)
    assert frirl_amd.learn_supported(prob, agent)
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=hc.TRAJ_EPISODES[env], budget=budget)
    torch.cuda.synchronize()
    assert (run.conv.converged == r["converged"]).all() and (run.conv.episodes == r["episodes"]).all(), run.conv.episodes.tolist()
    check_trajectory(r, prob, envs, run.steps_total, E)
    w = run.work.cpu().numpy()
    assert (w == w[0]).all()
    print(env, name, slices, budget, "extra rule visits", int(w[0, 1]), "oracle: rules summed over spreads", r["spread"]["spread_rules"],
          "over out-of-bounds updates", r["spread"]["outside_rules"])
    if name in ("thr0", "thr_small"):
        assert w[0, 1] > 0
    if name == "thr0":
        # work[:, 1] counts a rule base's size per extra sweep.  Greedy runs have two sources of them: the sweep of a snapped point
        # (only in updates whose qdiff lies outside the bounds, at most one each) and the spread's walk of every rule.  At threshold 0
        # the flags' bound is 0 = unknown, so every spread must walk every rule: the count is at least the oracle's rule count
        # summed over its spreads, and more than the snapped-point sweeps alone can account for.
        assert w[0, 1] >= r["spread"]["spread_rules"] > r["spread"]["outside_rules"], (w[0, 1], r["spread"])


@pytest.mark.parametrize("name", hc.NON_DEFAULT)
@pytest.mark.parametrize("nant,A", hc.EXTERNAL_SHAPES)
def test_caller_stepped_agents_follow_the_oracle(nant, A, name):
    """tests/test_hip_external.py::follow_the_oracle (frirl_hip_agent_begin / _observe, 16 agents, 4 episodes) with the description
    overridden by every set.  The tie rule is the existing one: a pick may follow the device inside a 1e-12 tie of the oracle, at most
    10 % of a case's picks.  Consequents at 1e-9, not follow_the_oracle's default 1e-6."""
    from tests.test_hip_external import follow_the_oracle, point_desc
    mirrors = follow_the_oracle(nant, A, 0, override=hc.overrides(name, point_desc(nant, A), point=True), tol=TOL)
    ties, picks = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    assert ties * 10 <= picks, (ties, picks)
    assert all(m.oa.skip_rules == hc.point_desc(nant, A, name)["skip_rules"] and m.oa.weight_thr == hc.point_desc(nant, A, name)["weight_thr"] for m in mirrors)


TEACH_CASES = [(nant, A, name, maxR) for nant, A in hc.TEACH_SHAPES for name in hc.TEACH_SETS for maxR in (512, 2304)] + [(6, 11, "thr_small", 17408)]


@pytest.mark.parametrize("nant,A,name,maxR", TEACH_CASES)
def test_replay_follows_the_oracle_over_the_sets(nant, A, name, maxR):
    """tests/test_hip_teach.py::test_replay_follows_the_oracle_on_new_shapes (forced actions: no arg-max, no ties) with the description
    overridden: the one-wave kernel (maxR 512), the 256-thread kernel (2304) and once the tracked candidates (17408).  Consequents at 1e-9,
    not assert_matches_mirrors' default 1e-6."""
    from tests import teach_ref as tr
    from tests.test_hip_teach import assert_matches_mirrors, demonstration, device_log
    d, log = tr.point_case(nant, A, hparams=name)
    mirrors = tr.mirrors_for(d, log, maxR)
    consumed = [m.replay(log, e) for e, m in enumerate(mirrors)]
    prob, agent, envs = frirl_amd.fresh_batch(d, len(mirrors), maxR, DEV)
    assert agent.desc.skip_rules == d["skip_rules"] and agent.desc.weight_significant == d["weight_thr"]
    replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, demonstration(device_log(log)))
    assert replayed.cpu().tolist() == consumed and refused.cpu().tolist() == [m.refused for m in mirrors]
    assert_matches_mirrors(d, prob, envs, mirrors, (nant, A, name, maxR), tol=TOL)


@pytest.mark.parametrize("weight_thr", [0.002, 0.3])
@pytest.mark.parametrize("nant", [3, 5])
def test_weights_from_spread_and_merge_rb_at_other_thresholds(nant, weight_thr):
    """tests/test_hip_power.py::test_weights_from_spread_and_merge_rb_at_power_2 at the default power with weight_significant 0.002 and
    0.3.  frirl_hip_weights_from_spread takes no agent and never sees the threshold: its half only sets the merge up, as there, and
    repeats that test's weights check at the default power.  What depends on the set is frirl_hip_merge_rb (merge.hip overwrites every
    rule whose weight exceeds the threshold), against the oracle's merge_rb with an agent of the same values."""
    import ctypes as C
    import torch
    from tests.test_hip_power import RTOL, merge_case
    b, grids, hp, oag, srant, srconc, spread, fives = merge_case(nant, 0, weight_thr=weight_thr)
    assert oag.weight_thr == weight_thr and hp["weight_thr"] == weight_thr
    E, maxR = 2, b.maxR
    prob = b.to_device(compressed=True)
    grid_div = [float(g[1] - g[0]) for g in grids]
    agent = frirl_amd.Agent(DEV, nant, grids, grid_div, [0.0] * nant, b.ve[nant - 1, ::4], hp["alpha"], hp["gamma"], hp["qdiff_pos"], hp["qdiff_neg"],
                            hp["weight_thr"], hp["skip_rules"], 0, frirl_amd.ENV_EXTERNAL)
    store = torch.zeros((E, nant, maxR), dtype=torch.float64, device=DEV)
    for e in range(E):
        n = int(b.nrules[e])
        store[e, :, :n] = dev(b.u[np.arange(nant)[:, None], b.uidx[e, :, :n]])
    envs = frirl_amd.Envs(prob, DEV, rant_init=store)
    envs.spread_ant.copy_(dev(spread))
    envs.spread_R.copy_(dev(b.nrules))
    weights = torch.zeros((E, maxR), dtype=torch.float64, device=DEV)
    frirl_amd.check(frirl_amd.lib().frirl_hip_weights_from_spread(C.byref(prob.tables), C.byref(prob.bases), 0, C.byref(envs.desc),
                                                                  C.c_void_p(weights.data_ptr()), None), "frirl_hip_weights_from_spread")
    torch.cuda.synchronize()
    w = weights.cpu().numpy()
    for e in range(E):
        n = int(b.nrules[e])
        assert rel(w[e, :n], fives[e].weights[:n]).max() <= RTOL, e
        assert (w[e, n:] == 0).all() and int(envs.spread_R[e]) == 0
    R_before = [f.R for f in fives]
    q_before = [np.array(f.rconc[: f.R]).copy() for f in fives]
    full = prob.merge_rb(agent, dev(srant), dev(srconc), weights, rant_store=store)
    torch.cuda.synchronize()
    assert (full.cpu().numpy() == 0).all()
    nr, rb, st = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), store.cpu().numpy()
    inserted = changed = 0
    for e in range(E):
        f = fives[e]
        f.merge_rb(oag, srant, srconc)
        R1 = f.R
        assert nr[e] == R1, (e, nr[e], R1)
        assert (st[e, :, :R1].T == np.array(f.rant[:R1])).all(), "antecedents / rule order"
        assert (rb[e, :nant, :R1] == np.array(f.veval[:, :R1])).all()
        ref = np.array(f.rconc[:R1])
        assert rel(rb[e, nant, :R1], ref).max() <= TOL, e
        inserted += R1 - R_before[e]
        changed += int((ref[: R_before[e]] != q_before[e]).sum())
    assert inserted > 0 and changed > 0, (inserted, changed)
