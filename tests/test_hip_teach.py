"""Imitation on the GPU: teacher actions in the caller-stepped loop (frirl_hip_agent_begin_taught / _observe_taught) and the one-launch
replay of recorded demonstrations (frirl_hip_learn_demonstration).

1. No teacher (NULL, or -1 everywhere) gives the bits of frirl_hip_agent_begin / _observe after every step.
2. A teacher that repeats the agent's own picks changes nothing.
3. Forced actions, record by record, against the oracle (tests/teach_ref.py: TaughtMirror), new shapes up to A = 32, one at power 2.
4. Mixed rows: forced and free rows of one batch are the rows of an all-forced and an all-free batch.
5. The replay equals the per-record chain of taught calls: decisions and integer state exactly, consequents within the contract.
6. The replay against the oracle, new shapes and the three demos' logs.
7. 65 536 agents in one launch.
"""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from tests import teach_ref as tr
from tests.test_hip_external import PointEnv, assert_same, diversified_starts, generic_quantize, point_desc, state_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONTRACT = 1e-6       # |q - ref| <= 1e-6 * max(|ref|, 1e-9): the project's contract for interpolated values (test_hip_external.py)


def within_contract(q, ref, tol=CONTRACT):
    return np.abs(q - ref) <= tol * np.maximum(np.abs(ref), 1e-9)


# ---- 1, 2: the taught entry points without a teacher's say --------------------------------------------------------------------
def taught_symbol(begin, prob, agent, envs, obs, reward=None, success=None, q_obs=None, teacher=None):
    """The _taught symbols called directly, so that teacher = NULL reaches them (frirl_amd.agent_begin / _observe call the untaught
    symbols when no teacher is given)."""
    io, action, action_idx = frirl_amd._agent_io(prob, obs, q_obs, reward, success)
    fn = frirl_amd.lib().frirl_hip_agent_begin_taught if begin else frirl_amd.lib().frirl_hip_agent_observe_taught
    frirl_amd.check(fn(C.byref(prob.tables), C.byref(prob.bases), C.byref(agent.desc), C.byref(envs.desc), C.byref(io), frirl_amd._ptr(teacher),
                       frirl_amd._stream()), "taught")
    return action, action_idx


NO_TEACHER = {
    "mountaincar-explore": dict(env="mountaincar", maxR=512, epsilon=0.2, no_random=0),     # one-wave kernels, exploring
    "acrobot-large": dict(env="acrobot", maxR=17408, epsilon=0.0, no_random=1),             # 256 threads, index mirror, TRACK
}


@pytest.mark.parametrize("cfg", list(NO_TEACHER))
def test_no_teacher_changes_nothing(cfg):
    import torch
    c = NO_TEACHER[cfg]
    d = frirl_amd.demo_describe(c["env"])
    E, max_steps = 64, 50
    ss = torch.from_numpy(diversified_starts(d, E, 7)).to(DEV)
    kw = dict(max_steps=max_steps, epsilon=c["epsilon"], no_random=c["no_random"], seed=11)
    runs = [frirl_amd.fresh_batch(d, E, c["maxR"], DEV, **kw) for _ in range(3)]      # untaught, teacher NULL, teacher -1 everywhere
    minus = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    teachers = [None, None, minus]
    for ep in range(2):
        acts = []
        for i, (p, a, e) in enumerate(runs):
            acts.append(frirl_amd.agent_begin(p, a, e, ss) if i == 0 else taught_symbol(True, p, a, e, ss, teacher=teachers[i]))
        for t in range(max_steps + 1):
            for i in (1, 2):
                assert_same(state_arrays(runs[0][0], runs[0][2]), state_arrays(runs[i][0], runs[i][2]), (cfg, ep, t, i))
            live = runs[0][2].done == 0
            for i in (1, 2):
                assert torch.equal(acts[0][0][live].view(torch.int64), acts[i][0][live].view(torch.int64)) and torch.equal(acts[0][1][live], acts[i][1][live])
            if t == max_steps:
                break
            for i, (p, a, e) in enumerate(runs):
                keep = acts[i]
                obs, reward, success, _ = frirl_amd.env_step(a, keep[0], e.states)
                new = frirl_amd.agent_observe(p, a, e, obs, reward, success) if i == 0 else taught_symbol(False, p, a, e, obs, reward, success, teacher=teachers[i])
                acts[i] = (torch.where(live, new[0], keep[0]), torch.where(live, new[1], keep[1]))
        assert bool((runs[0][2].done != 0).all())


def test_teacher_repeating_the_agents_own_picks_changes_nothing():
    import torch
    d = frirl_amd.demo_describe("mountaincar")
    E, max_steps = 64, 50
    ss = torch.from_numpy(diversified_starts(d, E, 3)).to(DEV)
    kw = dict(max_steps=max_steps, epsilon=0.2, no_random=0, seed=5)
    (pa, aa, ea), (pb, ab, eb) = (frirl_amd.fresh_batch(d, E, 512, DEV, **kw) for _ in range(2))
    for ep in range(2):
        act_a, idx_a = frirl_amd.agent_begin(pa, aa, ea, ss)
        act_b, idx_b = frirl_amd.agent_begin(pb, ab, eb, ss, teacher=idx_a)
        for t in range(max_steps):
            assert_same(state_arrays(pa, ea), state_arrays(pb, eb), (ep, t))
            live = ea.done == 0
            assert torch.equal(idx_a[live], idx_b[live])
            obs, reward, success, _ = frirl_amd.env_step(aa, act_a, ea.states)
            na, nia = frirl_amd.agent_observe(pa, aa, ea, obs, reward, success)
            act_a, idx_a = torch.where(live, na, act_a), torch.where(live, nia, idx_a)
            obs, reward, success, _ = frirl_amd.env_step(ab, act_b, eb.states)
            nb, nib = frirl_amd.agent_observe(pb, ab, eb, obs, reward, success, teacher=torch.where(live, idx_a, torch.full_like(idx_a, -1)))
            act_b, idx_b = torch.where(live, nb, act_b), torch.where(live, nib, idx_b)
        assert_same(state_arrays(pa, ea), state_arrays(pb, eb), (ep, "end"))


# ---- logs on the device, the per-record chain ---------------------------------------------------------------------------------
def device_log(log, rows=None):
    import torch
    out = {}
    for k in ("obs", "q_obs", "action", "reward", "success", "start", "length"):
        v = log[k]
        if v is not None and rows is not None:
            v = v[rows]
        out[k] = None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    return out


def demonstration(dl, q_obs=True, start=True, length=True):
    return frirl_amd.Demonstration(dl["obs"], dl["action"], dl["reward"], dl["success"], q_obs=dl["q_obs"] if q_obs else None,
                                   start=dl["start"] if start else None, length=dl["length"] if length else None)


def chain(prob, agent, envs, dl, passes=1, q_obs=True, on_record=None):
    """The per-record meaning of frirl_hip_learn_demonstration (include/frirl_hip.h) spelled out with the taught calls: a start record is
    agent_begin with a reset mask and the logged action as teacher, any other record agent_observe with it; rows whose log has ended
    (length, an out-of-range action) sit the call out behind done = 1, restored afterwards.  Returns (replayed, refused)."""
    import torch
    E, A = prob.E, agent.A
    L, T = dl["action"].shape
    sel = (lambda x, r: x[:, r].expand(E, *x.shape[2:]).contiguous()) if L == 1 else (lambda x, r: x[:, r].contiguous())
    length = dl["length"] if dl["length"] is not None else torch.full((E,), T, dtype=torch.int32, device=DEV)
    stopped = torch.zeros((E,), dtype=torch.bool, device=DEV)
    replayed = torch.zeros((E,), dtype=torch.int32, device=DEV)
    refused = torch.zeros((E,), dtype=torch.uint8, device=DEV)
    for _ in range(passes):
        for r in range(T):
            a = sel(dl["action"], r)
            active = (length > r) & ~stopped
            bad = active & ((a < 0) | (a >= A))
            stopped |= bad
            active &= ~bad
            starts = active & ((sel(dl["start"], r) != 0) if (dl["start"] is not None and r > 0) else torch.full_like(active, r == 0))
            obs = sel(dl["obs"], r)
            frirl_amd.agent_begin(prob, agent, envs, obs, reset=starts.to(torch.uint8), teacher=a)
            steps = active & ~starts
            done0, status0 = envs.done.clone(), envs.status.clone()
            envs.done.masked_fill_(~steps, 1)
            frirl_amd.agent_observe(prob, agent, envs, obs, sel(dl["reward"], r), sel(dl["success"], r),
                                    q_obs=sel(dl["q_obs"], r) if (q_obs and dl["q_obs"] is not None) else None, teacher=a)
            envs.done.copy_(torch.where(steps, envs.done, done0))
            envs.status.copy_(torch.where(steps, envs.status, status0))
            refused |= (steps & (envs.status == frirl_amd.UPD_FULL)).to(torch.uint8)
            replayed += active.to(torch.int32)
            if on_record is not None:
                on_record(r, active, envs.status.clone())
    return replayed, refused


EXACT_KEYS = ("nrules", "uidx", "rant", "q_ant", "states", "fus", "done", "ep_steps", "status", "episode")
worst = {}            # largest relative difference replay vs chain per scenario (printed; profiles/r14_teach.md records a run)


def assert_replay_equals_chain(pa, ea, pb, eb, where):
    """a = the replay, b = the chain: decisions and integer state exactly (rule counts, antecedents in every form, statuses, counters,
    the spread bookkeeping), consequents and ep_reward within the contract.  Returns the largest relative difference."""
    import torch
    sa, sb = state_arrays(pa, ea), state_arrays(pb, eb)
    assert_same({k: sa[k] for k in EXACT_KEYS}, {k: sb[k] for k in EXACT_KEYS}, where)
    assert torch.equal(ea.spread_R, eb.spread_R) and torch.equal(ea.spread_ant.view(torch.int64), eb.spread_ant.view(torch.int64)), where
    nant = pa.nant
    assert torch.equal(pa.rb[:, :nant].contiguous().view(torch.int64), pb.rb[:, :nant].contiguous().view(torch.int64)), where
    q, ref = pa.rb[:, nant].cpu().numpy(), pb.rb[:, nant].cpu().numpy()
    assert within_contract(q, ref).all(), where
    r, rref = ea.ep_reward.cpu().numpy(), eb.ep_reward.cpu().numpy()
    assert within_contract(r, rref).all(), where
    rel = float((np.abs(q - ref) / np.maximum(np.abs(ref), 1e-9)).max())
    worst[where] = max(worst.get(where, 0.0), rel)
    print(f"replay vs chain {where}: largest relative difference of a consequent {rel:.3e}")
    return rel


def replay_and_chain(d, log, maxR, where, p=0, passes=1, q_obs=True, start=True, length=True, rows=None, E=None, **agent_kw):
    dl = device_log(log, rows)
    E = E if E is not None else dl["action"].shape[0]
    if dl["length"].shape[0] != E:
        dl["length"] = dl["length"][:1].expand(E).contiguous()
    if not length:
        dl["length"] = None
    if not start:
        dl["start"] = None
    pa, aa, ea = frirl_amd.fresh_batch(d, E, maxR, DEV, p=p, **agent_kw)
    pb, ab, eb = frirl_amd.fresh_batch(d, E, maxR, DEV, p=p, **agent_kw)
    got = frirl_amd.learn_demonstration(pa, aa, ea, demonstration(dl, q_obs=q_obs, start=start, length=length), passes=passes)
    want = chain(pb, ab, eb, dl, passes=passes, q_obs=q_obs)
    import torch
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), where
    assert_replay_equals_chain(pa, ea, pb, eb, where)
    return (pa, aa, ea), got, dl


# ---- 3: forced actions against the oracle -------------------------------------------------------------------------------------
def assert_matches_mirrors(d, prob, envs, mirrors, where, statuses=True, tol=CONTRACT):
    nant = d["nant"]
    rant, rb, nrules = envs.rant.cpu().numpy(), prob.rb.cpu().numpy(), prob.nrules.cpu().numpy()
    steps, reward, status, fus, done, episode = (x.cpu().numpy() for x in (envs.ep_steps, envs.ep_reward, envs.status, envs.fus, envs.done, envs.episode))
    for e, m in enumerate(mirrors):
        R = m.five.R
        assert int(nrules[e]) == R, (where, e)
        assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all(), (where, e)
        assert int(steps[e]) == m.steps and float(reward[e]) == m.total and int(done[e]) == m.done and int(episode[e]) == m.episode_no, (where, e)
        assert int(fus[e]) == int(m.fus) and (not statuses or int(status[e]) == m.status), (where, e)
        q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
        assert within_contract(q, ref, tol).all(), (where, e)


FORCED = [(2, 3, 0), (2, 11, 0), (4, 3, 0), (4, 11, 0), (6, 3, 0), (6, 11, 0), (8, 3, 0), (8, 11, 0), (3, 32, 0), (4, 11, 2)]


@pytest.mark.parametrize("nant,A,p", FORCED)
def test_forced_actions_follow_the_oracle(nant, A, p):
    """Every action of the chain is the log's, so no pick and no tie rule is involved: rule count, antecedents, the status after every
    record, steps and rewards exactly, consequents within the contract."""
    d, log = tr.point_case(nant, A)
    maxR = 512
    mirrors = tr.mirrors_for(d, log, maxR, p=p)
    for e, m in enumerate(mirrors):
        m.replay(log, e)
    prob, agent, envs = frirl_amd.fresh_batch(d, len(mirrors), maxR, DEV, p=p)
    seen = []
    chain(prob, agent, envs, device_log(log), on_record=lambda r, active, status: seen.append((active.cpu().numpy(), status.cpu().numpy())))
    for e, m in enumerate(mirrors):
        got = [int(st[e]) for act, st in seen if act[e]]
        assert got == m.trace, (nant, A, p, e)
    assert_matches_mirrors(d, prob, envs, mirrors, (nant, A, p))
    assert sum(m.branches[tr.INSERTED] for m in mirrors) > 0 and sum(m.branches[tr.SPREAD] for m in mirrors) > 0


# ---- 4: mixed rows ------------------------------------------------------------------------------------------------------------
def test_forced_and_free_rows_do_not_see_each_other():
    import torch
    nant, A, E = 4, 5, 64
    d = dict(point_desc(nant, A), max_steps=30)
    env = PointEnv(nant - 1)
    rng = np.random.default_rng(9)
    s0 = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    s1 = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    mask = torch.from_numpy(rng.uniform(size=E) < 0.4).to(DEV)
    odd = (torch.arange(E, device=DEV) % 2) == 1
    rows = torch.arange(E, device=DEV, dtype=torch.int32)
    forced = lambda t: ((rows * 3 + t) % A).to(torch.int32)                                      # noqa: E731
    teacher = {"mixed": lambda t: torch.where(odd, forced(t), torch.full_like(rows, -1)), "forced": forced, "free": lambda t: None}
    kw = dict(epsilon=0.2, no_random=0, seed=77)          # the free rows explore: their stream position must not depend on the others
    runs = {k: list(frirl_amd.fresh_batch(d, E, 512, DEV, **kw)) for k in teacher}
    for k, r in runs.items():
        act, idx = frirl_amd.agent_begin(r[0], r[1], r[2], s0, teacher=teacher[k](0))
        r.append(act)
        if k != "free":
            took = idx == forced(0)
            assert bool(took.all() if k == "forced" else took[odd].all())

    def compare(where):
        sm, sf, sn = (state_arrays(runs[k][0], runs[k][2]) for k in ("mixed", "forced", "free"))
        assert_same(sm, sf, (where, "odd rows"), rows=odd)
        assert_same(sm, sn, (where, "even rows"), rows=~odd)
        assert torch.equal(runs["mixed"][3][odd], runs["forced"][3][odd]) and torch.equal(runs["mixed"][3][~odd], runs["free"][3][~odd])

    for t in range(1, 41):
        compare(t)
        if t == 12:             # a reset mask in the middle of the episodes
            for k, r in runs.items():
                act, _ = frirl_amd.agent_begin(r[0], r[1], r[2], s1, reset=mask.to(torch.uint8), teacher=teacher[k](100))
                r[3] = torch.where(mask, act, r[3])
            compare("reset")
        for k, r in runs.items():
            prob, agent, envs, act = r
            live = envs.done == 0
            obs, reward, success = env.step(torch, envs.states, act)
            nxt, _ = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32), teacher=teacher[k](t))
            r[3] = torch.where(live, nxt, act)
    compare("end")


# ---- 5: the replay equals the chain -------------------------------------------------------------------------------------------
def with_q_obs(d, log):
    """The log with the generic quantiser's q_obs spelled out on the host."""
    q = np.zeros_like(log["obs"])
    for e in range(q.shape[0]):
        for r in range(q.shape[1]):
            q[e, r] = generic_quantize(d, log["obs"][e, r])
    return dict(log, q_obs=q)


def test_replay_one_wave_and_256_threads():
    """point 4 x 3 at maxR = 512 (one wave) and 2304 (256 threads, index mirror); the logs hold an episode boundary inside, records
    after done, and records whose state cell and action repeat (tests/test_teach_ref.py); rule counts end odd and even."""
    d, log = tr.point_case(4, 3)
    counts = []
    for maxR in (512, 2304):
        (prob, _, envs), (replayed, refused), dl = replay_and_chain(d, log, maxR, f"point4x3 maxR={maxR}")
        assert (replayed.cpu().numpy() == log["length"]).all() and int(refused.sum()) == 0
        counts.append(prob.nrules.cpu().numpy())
    assert (counts[0] == counts[1]).all() and (counts[0] % 2 == 0).any() and (counts[0] % 2 == 1).any()


def test_replay_with_tracked_spread_candidates():
    """acrobot at maxR = 17 408: 256 threads, index mirror, spread candidates tracked in the pair sweep; q_obs given."""
    d, log = tr.demo_case("acrobot")
    replay_and_chain(d, log, 17408, "acrobot maxR=17408")


def test_replay_with_tracked_spread_candidates_without_the_mirror_cases():
    """More tracked forms at maxR = 17 408: a 4-antecedent PointEnv shape at run-time power 2 and at the default power (index mirror,
    11 actions: the per-step chain does not track there, the replay does), and the 3-antecedent shape with 32 actions."""
    d, log = tr.point_case(4, 11)
    replay_and_chain(d, log, 17408, "point4x11 p=2 maxR=17408", p=2)
    replay_and_chain(d, log, 17408, "point4x11 maxR=17408")
    d, log = tr.point_case(3, 32)
    replay_and_chain(d, log, 17408, "point3x32 maxR=17408")


@pytest.mark.parametrize("p", [2, 6])
def test_replay_at_other_shepard_powers(p):
    d, log = tr.point_case(4, 11)
    replay_and_chain(d, log, 512, f"point4x11 p={p}", p=p)
    replay_and_chain(d, log, 2304, f"point4x11 p={p} maxR=2304", p=p)


@pytest.mark.parametrize("case", ["point4x3", "cartpole"])
def test_replay_on_rule_bases_that_fill_mid_log(case):
    d, log = tr.point_case(4, 3) if case == "point4x3" else tr.demo_case("cartpole")
    maxR = 2 ** d["nant"] + 8
    (prob, _, envs), (replayed, refused), _ = replay_and_chain(d, log, maxR, f"{case} maxR={maxR}")
    refused, nrules = refused.cpu().numpy(), prob.nrules.cpu().numpy()
    assert refused.sum() > 0 and (nrules[refused == 1] == maxR).all()
    mirrors = tr.mirrors_for(d, log, maxR)
    for e, m in enumerate(mirrors):
        m.replay(log, e)
    assert (refused == np.array([m.refused for m in mirrors])).all()
    assert_matches_mirrors(d, prob, envs, mirrors, case)


def test_replay_lengths_differ_per_agent():
    d, log = tr.point_case(6, 3)
    E = log["action"].shape[0]
    short = dict(log, length=np.minimum(log["length"], np.array([1, 2, 0, 17, 66, 1000, 5, 70][:E], dtype=np.int32)))
    (prob, _, envs), (replayed, _), _ = replay_and_chain(d, short, 512, "point6x3 lengths")
    assert (replayed.cpu().numpy() == short["length"]).all()
    assert int(envs.episode[2]) == 0 and int(envs.episode[0]) == 1 and int(envs.ep_steps[0]) == 0 and int(envs.ep_steps[1]) == 1


def test_replay_of_a_single_record():
    d, log = tr.point_case(4, 3)
    one = {k: (v[:, :1] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in log.items()}
    one["length"] = np.ones_like(log["length"])
    (prob, _, envs), (replayed, _), _ = replay_and_chain(d, one, 512, "point4x3 T=1", start=False, length=False)
    assert bool((replayed == 1).all()) and bool((envs.episode == 1).all()) and bool((prob.nrules == 16).all())


def test_replay_of_one_shared_log():
    """agent_stride = 0: every agent replays agent 3's log; all end with the same rule base."""
    import torch
    d, log = tr.point_case(4, 11)
    (prob, _, envs), (replayed, _), dl = replay_and_chain(d, log, 512, "point4x11 shared", rows=slice(3, 4), E=8)
    assert dl["action"].shape[0] == 1 and bool((replayed == int(log["length"][3])).all())
    assert bool((prob.rb == prob.rb[:1]).all()) and bool((prob.nrules == prob.nrules[0]).all())
    mirror = tr.mirrors_for(d, log, 512)[3]
    mirror.replay(log, 3)
    assert int(prob.nrules[5]) == mirror.five.R


@pytest.mark.parametrize("env", ["mountaincar", "acrobot"])
def test_replay_with_and_without_the_callers_q_obs(env):
    """The oracle's quantiser of these two demos is the generic grid rule, so q_obs = NULL must give what the logged q_obs gives."""
    d, log = tr.demo_case(env)
    (pa, _, ea), _, _ = replay_and_chain(d, log, 512, f"{env} q_obs given", q_obs=True)
    (pb, _, eb), _, _ = replay_and_chain(d, log, 512, f"{env} q_obs NULL", q_obs=False)
    assert_same(state_arrays(pa, ea), state_arrays(pb, eb), env)


def test_replay_with_q_obs_spelled_out_for_a_new_shape():
    d, log = tr.point_case(6, 11)
    (pa, _, ea), _, _ = replay_and_chain(d, log, 512, "point6x11 q_obs NULL", q_obs=False)
    (pb, _, eb), _, _ = replay_and_chain(d, with_q_obs(d, log), 512, "point6x11 q_obs given", q_obs=True)
    assert_same(state_arrays(pa, ea), state_arrays(pb, eb), "point6x11")


def test_replay_stops_before_an_out_of_range_action():
    d, log = tr.point_case(4, 3)
    bad = dict(log, action=log["action"].copy())
    bad["action"][0, 17], bad["action"][1, 0], bad["action"][2, 40], bad["action"][3, int(log["length"][3]) - 1] = d["A"], -1, 32, 1 << 20
    (prob, _, envs), (replayed, _), _ = replay_and_chain(d, bad, 512, "point4x3 bad action", passes=2)
    want = 2 * log["length"]
    want[:4] = [17, 0, 40, log["length"][3] - 1]
    assert (replayed.cpu().numpy() == want).all()
    assert int(envs.episode[1]) == 0 and int(prob.nrules[1]) == 16 and int(envs.status[1]) == 0       # agent 1 consumed nothing: untouched


def test_two_passes_are_two_calls():
    import torch
    d, log = tr.point_case(4, 11)
    (pa, _, ea), (replayed, _), dl = replay_and_chain(d, log, 512, "point4x11 passes=2", passes=2)
    pb, ab, eb = frirl_amd.fresh_batch(d, pa.E, 512, DEV)
    demo = demonstration(dl)
    r1, _ = frirl_amd.learn_demonstration(pb, ab, eb, demo)
    r2, _ = frirl_amd.learn_demonstration(pb, ab, eb, demo)
    assert torch.equal(r1 + r2, replayed)
    assert_same(state_arrays(pa, ea), state_arrays(pb, eb), "passes=2 vs two calls")


def test_replay_under_evaluate_learns_nothing():
    d, log = tr.point_case(4, 3)
    (prob, _, envs), (replayed, refused), _ = replay_and_chain(d, log, 512, "point4x3 evaluate", evaluate=1)
    assert bool((prob.nrules == 16).all()) and bool((prob.rb[:, 4] == 0).all()) and int(refused.sum()) == 0
    assert (replayed.cpu().numpy() == log["length"]).all() and bool((envs.done == 1).all())


# ---- 6: the replay against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nant,A,p", FORCED)
def test_replay_follows_the_oracle_on_new_shapes(nant, A, p):
    d, log = tr.point_case(nant, A)
    mirrors = tr.mirrors_for(d, log, 512, p=p)
    consumed = [m.replay(log, e) for e, m in enumerate(mirrors)]
    prob, agent, envs = frirl_amd.fresh_batch(d, len(mirrors), 512, DEV, p=p)
    replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, demonstration(device_log(log)))
    assert replayed.cpu().tolist() == consumed and refused.cpu().tolist() == [m.refused for m in mirrors]
    assert_matches_mirrors(d, prob, envs, mirrors, (nant, A, p))


@pytest.mark.parametrize("env", ["mountaincar", "acrobot", "cartpole"])
@pytest.mark.parametrize("maxR", [512, 2304])
def test_replay_follows_the_oracle_on_the_demos_logs(env, maxR):
    d, log = tr.demo_case(env)
    mirrors = tr.mirrors_for(d, log, maxR)
    consumed = [m.replay(log, e, passes=2) for e, m in enumerate(mirrors)]
    prob, agent, envs = frirl_amd.fresh_batch(d, len(mirrors), maxR, DEV)
    replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, demonstration(device_log(log)), passes=2)
    assert replayed.cpu().tolist() == consumed and refused.cpu().tolist() == [m.refused for m in mirrors]
    assert_matches_mirrors(d, prob, envs, mirrors, (env, maxR))


# ---- 7: scale -----------------------------------------------------------------------------------------------------------------
def test_65536_agents_in_one_launch():
    import torch
    nant, A, E, T = 3, 5, 65536, 8
    d = dict(point_desc(nant, A), max_steps=3)
    maxR = 2 ** nant + 4
    g = torch.Generator(device=DEV).manual_seed(21)
    rnd = lambda *shape: torch.rand(shape, generator=g, device=DEV, dtype=torch.float64)        # noqa: E731
    obs = (rnd(E, T, nant - 1) * 1.8 - 0.9).contiguous()
    action = (rnd(E, T) * A).to(torch.int32).clamp_(0, A - 1)
    reward = (rnd(E, T) * 40.0 - 30.0).contiguous()
    success = (rnd(E, T) < 0.15).to(torch.int32)
    start = (rnd(E, T) < 0.2).to(torch.uint8)
    length = (1 + (rnd(E) * T).to(torch.int32)).clamp_(1, T)
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV)
    replayed, refused = frirl_amd.learn_demonstration(prob, agent, envs, frirl_amd.Demonstration(obs, action, reward, success, start=start, length=length))
    torch.cuda.synchronize()
    # the bookkeeping restated with tensor operations
    done, steps = torch.zeros((E,), dtype=torch.int32, device=DEV), torch.zeros((E,), dtype=torch.int32, device=DEV)
    total, episode = torch.zeros((E,), dtype=torch.float64, device=DEV), torch.zeros((E,), dtype=torch.int32, device=DEV)
    states = torch.zeros((E, nant - 1), dtype=torch.float64, device=DEV)
    stepped = torch.zeros((E,), dtype=torch.int32, device=DEV)
    for r in range(T):
        active = length > r
        st = active & ((start[:, r] != 0) if r > 0 else torch.ones_like(active))
        step = active & ~st & (done == 0)
        done = torch.where(st, torch.zeros_like(done), done)
        steps = torch.where(st, torch.zeros_like(steps), steps) + step.to(torch.int32)
        total = torch.where(st, torch.zeros_like(total), total)
        total = torch.where(step, total + reward[:, r], total)
        episode += st.to(torch.int32)
        states = torch.where((st | step)[:, None], obs[:, r], states)
        done = torch.where(step & ((success[:, r] == 1) | (steps >= d["max_steps"])), torch.ones_like(done), done)
        stepped += step.to(torch.int32)
    assert torch.equal(replayed, length), "a row was left untouched or over-run"
    assert torch.equal(envs.done, done) and torch.equal(envs.ep_steps, steps) and torch.equal(envs.episode, episode)
    assert torch.equal(envs.ep_reward.view(torch.int64), total.view(torch.int64)) and torch.equal(envs.states.view(torch.int64), states.view(torch.int64))
    nrules, status = prob.nrules, envs.status
    assert bool((nrules >= 2 ** nant).all()) and bool((nrules <= maxR).all()) and bool((nrules - 2 ** nant <= stepped).all())
    assert bool(((status >= frirl_amd.UPD_INACTIVE) & (status <= frirl_amd.UPD_FULL)).all())
    assert bool((nrules[refused == 1] == maxR).all()) and bool((refused[stepped == 0] == 0).all()) and int(refused.sum()) > 0
    assert bool((envs.episode >= 1).all()) and int((stepped > 0).sum()) > E // 2 and int((length == T).sum()) > 0
