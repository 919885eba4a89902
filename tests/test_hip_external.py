"""The caller's-environment API on the GPU (frirl_hip_agent_begin / frirl_hip_agent_observe, frirl_episode.c:28-194 with the
environment outside the kernel).

1. Driving a demo through it -- frirl_hip_env_step playing the caller's environment -- gives the bits of the fused demo kernels
   (frirl_hip_episode_begin / _step) after every step, for the one-wave, the 256-thread and the TRACK kernels, with exploration.
2. New shapes (nant 2..8, A 3 / 5 / 11) of an environment written in torch, against a per-agent mirror built from the oracle's
   pieces (Five.best_action, Five.update_sarsa, the generic quantiser restated), whole construct loops.
3. A reset mask restarts only the selected rows.
4. 65 536 agents, rule bases that fill up (FRIRL_HIP_UPD_FULL), consistent bookkeeping.
"""
import math

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import explore_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def diversified_starts(d, E, seed):
    """Start states spread over each state grid's range (the reference diversifies them per agent, frirl_agent.c:121-139)."""
    rng = np.random.default_rng(seed)
    cols = []
    for k in range(d["nstates"]):
        g = d["grids"][k]
        lo, hi = float(g.min()), float(g.max())
        cols.append(d["values_def"][k] + rng.uniform(-0.1, 0.1, E) * (hi - lo) if hi > lo else np.full(E, d["values_def"][k]))
    return np.ascontiguousarray(np.stack(cols, 1))


def state_arrays(prob, envs):
    return dict(rb=prob.rb, nrules=prob.nrules, uidx=prob.uidx, rant=envs.rant, q_ant=envs.q_ant, states=envs.states, fus=envs.fus,
                done=envs.done, ep_steps=envs.ep_steps, ep_reward=envs.ep_reward, status=envs.status, episode=envs.episode)


def assert_same(a, b, where, rows=None):
    import torch
    for k in a:
        x, y = a[k], b[k]
        if rows is not None:
            x, y = x[rows], y[rows]
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), (where, k)


# ---- 1. bit identity with the fused demo kernels -------------------------------------------------------------------------
CONFIGS = {
    "explore": dict(maxR=512, epsilon=0.2, no_random=0),      # one-wave kernels, epsilon-greedy on the counter stream
    "small": dict(maxR=None, epsilon=0.0, no_random=1),       # one-wave kernels, rule bases that fill (FULL): 2^nant + 8 rules
    "large": dict(maxR=17408, epsilon=0.0, no_random=1),      # > 16 896: 256 threads, index mirror, TRACK where it applies
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("env", ["mountaincar", "cartpole", "acrobot"])
def test_observe_is_bit_identical_to_the_fused_step(env, cfg):
    import torch
    c = CONFIGS[cfg]
    d = frirl_amd.demo_describe(env)
    E, max_steps, episodes = 256, 120, 3
    if c["maxR"] is None:
        c = dict(c, maxR=2 ** d["nant"] + 8)
    ss = torch.from_numpy(diversified_starts(d, E, 7)).to(DEV)
    kw = dict(max_steps=max_steps, epsilon=c["epsilon"], no_random=c["no_random"], seed=11)
    pa, aa, ea = frirl_amd.fresh_batch(d, E, c["maxR"], DEV, start_states=ss, **kw)
    pb, ab, eb = frirl_amd.fresh_batch(d, E, c["maxR"], DEV, **kw)
    NS = d["nant"] - 1
    for ep in range(episodes):
        frirl_amd.episode_begin(pa, aa, ea)
        action, aidx = frirl_amd.agent_begin(pb, ab, eb, ss)
        assert_same(state_arrays(pa, ea), state_arrays(pb, eb), (ep, "begin"))
        assert torch.equal(action.view(torch.int64), ea.q_ant[:, NS].contiguous().view(torch.int64))
        assert torch.equal(ab.grid_values[NS][aidx.long()], action)
        for t in range(max_steps):
            was_done = eb.done.clone()
            frirl_amd.episode_step(pa, aa, ea)
            obs, reward, success, q_states = frirl_amd.env_step(ab, action, eb.states)
            nxt, nidx = frirl_amd.agent_observe(pb, ab, eb, obs, reward, success, q_obs=q_states if env == "cartpole" else None)
            assert_same(state_arrays(pa, ea), state_arrays(pb, eb), (ep, t))
            live = was_done == 0
            assert torch.equal(nxt[live].view(torch.int64), ea.q_ant[live, NS].contiguous().view(torch.int64)), (ep, t)
            action = torch.where(live, nxt, action)
            if bool((eb.done != 0).all()):
                break
        assert bool((eb.done != 0).all())
    if cfg == "small":
        assert int((pb.nrules == pb.maxR).sum()) > 0, "the small configuration should fill some rule bases"


# ---- 2. new shapes against the oracle -------------------------------------------------------------------------------------
class PointEnv:
    """A caller's environment with only + - * / and comparisons, so torch on the device and numpy on the host agree bit for bit:
    every state coordinate drifts towards 0 by 5 % per step and is pushed by the action with a per-dimension gain; reward
    -4 (sum of squares), success (+100) once every |x_k| < 0.12."""

    def __init__(self, ns):
        self.gain = [0.04 + 0.015 * k for k in range(ns)]
        self.ns = ns

    def step(self, xp, x, a):
        """xp = torch or numpy; x [E, ns], a [E] -> new x, reward, success (int32)."""
        cols, inside = [], None
        for k in range(self.ns):
            v = x[:, k] + a * self.gain[k]
            v = v - x[:, k] * 0.05
            v = xp.where(v < -1.0, -1.0 + 0.0 * v, v)
            v = xp.where(v > 1.0, 1.0 + 0.0 * v, v)
            cols.append(v)
            ok = (v < 0.12) & (v > -0.12)
            inside = ok if inside is None else (inside & ok)
        r = 0.0 - (cols[0] * cols[0]) * 4.0
        for k in range(1, self.ns):
            r = r - (cols[k] * cols[k]) * 4.0
        r = xp.where(inside, 100.0 + 0.0 * r, r)
        return xp.stack(cols, 1), r, inside


def point_desc(nant, A, U=41):
    ns = nant - 1
    # irregular, asymmetric grids: a symmetric toy problem has exact Q ties between actions in real arithmetic, which the reference's
    # sequential sums and the device's reduction tree (<= 1e-6 contract) break differently
    states = [dict(values=np.linspace(-0.9, 1.0, 5 + (k % 3)) + 0.011 * (np.arange(5 + (k % 3)) % 2), div=1.9 / (4 + (k % 3)), steep=1.0 + 0.5 * (k % 2),
                   default=0.0, universe_div=0.06) for k in range(ns)]
    # the action universe reaches past the action values, as in every demo: the reference snaps the actions' VE values with one
    # point fewer (frirl_init.c:156-158), so an action on the universe's last point would have two VE values
    actions = dict(values=np.linspace(-1.0, 1.0, A) + 0.0137 * (np.arange(A) % 3), div=2.0 / (A - 1), universe_div=0.1)
    return frirl_amd.describe(states, actions, U, 0.5, 1.0, 1.0, -1.0, reward_good_above=-1e9, qdiff_final_tolerance=5.0, max_steps=40,
                              name=f"point{nant}x{A}")


def c_round(y):
    r = math.floor(abs(y))
    if abs(y) - r >= 0.5:
        r += 1
    return r if y >= 0 else -r


def generic_quantize(d, s):
    """frirl_episode's generic quantize_observations of the reference's examples (the device's env_quantize, envs.h)."""
    q = np.zeros(len(s))
    for i in range(len(s)):
        g = d["grids"][i]
        where = int(c_round((s[i] + abs(g[0])) / d["grid_div"][i]))
        where = min(max(where, 0), len(g) - 1)
        q[i] = g[where]
    return q


class Mirror:
    """One agent of frirl_sequential_run's construct loop restated with the oracle's FIVE pieces."""

    def __init__(self, d, start, maxR, p=0, explore=None, gid=0):
        nant = d["nant"]
        self.explore, self.gid, self.episode_no = explore, gid, 0       # explore: dict(epsilon, seed, env_id_base) or None = greedy
        self.explored = self.changed = self.clamped = 0                  # picks on the random branch / that changed the action / clamped
        R0 = 2 ** nant
        rant0 = np.array([[d["grids"][k].min() if ((j // (R0 >> (k + 1))) % 2) == 0 else d["grids"][k].max() for k in range(nant)] for j in range(R0)])
        self.five = ob.Five(d["u"], d["ve"], nant, d["U"], maxR, rant=rant0, rconc=np.zeros(R0), p=p)
        self.oa = ob.Agent(d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"], d["weight_thr"], d["skip_rules"], d["grids"])
        self.d, self.start, self.fus = d, np.array(start), 0.0
        self.prev = dict(R=self.five.R, steps=-1, reward=-1.0, q=np.array(self.five.rconc[: maxR]).copy())
        self.converged = False
        self.ties = 0          # picks taken from the device (below)
        self.picks = 0         # picks made
        self.near = 0          # picks at which the oracle's own two best conclusions lie within 1e-12 relative

    def pick(self, states, device_pick, step=0):
        """Greedy action (frirl_get_best_action).  Where the oracle's conclusions tie the device's pick within 1e-12 relative --
        Q equal in real arithmetic, e.g. nant = 2, whose corner rules learn action-independent values -- the device's pick is
        followed: tie-breaking below the 1e-6 contract is not part of it.  Any other difference is a failure.
        With exploration the pick of tests/explore_ref.py at (episode, step) replaces the greedy one where the stream says so: such a
        pick is never a tie and never follows the device."""
        best, oc = self.five.best_action(states, self.d["action_ve"])
        self.picks += 1
        x = self.explore
        if x is not None and explore_ref.explores(x["epsilon"], 0, x["seed"], self.gid, self.episode_no, step):
            a, clamped = explore_ref.random_action(len(oc), x["seed"], self.gid, self.episode_no, step)
            self.explored += 1
            self.changed += int(a != best)
            self.clamped += int(clamped)
            return a
        srt = np.sort(oc)
        self.near += int(len(srt) > 1 and srt[-1] - srt[-2] <= 1e-12 * abs(srt[-1]))
        if device_pick is None:          # dry run on the CPU: the oracle alone
            return best
        if device_pick != best and abs(oc[device_pick] - oc[best]) <= 1e-12 * abs(oc[best]):
            self.ties += 1
            return device_pick
        return best

    def episode(self, env, picks):
        d, f = self.d, self.five
        NS = d["nant"] - 1
        av = d["grids"][NS]
        self.prev["R"], self.prev["q"] = f.R, np.array(f.rconc[: f.maxR]).copy()        # frirl_sequential_run.c:68-72
        self.episode_no += 1                                                               # frirl_hip_agent_begin: episode[e] + 1
        states = self.start.copy()
        picks = picks if picks is not None else [None] * (d["max_steps"] + 1)
        a0 = self.pick(states, picks[0], 0)                                                 # frirl_episode.c:78, un-quantised
        q_ant = np.concatenate([states, [av[a0]]])
        actions, steps, total = [a0], 0, 0.0
        while True:
            x, r, ok = env.step(np, states[None], np.array([q_ant[NS]]))
            cur, r, success = x[0], float(r[0]), int(ok[0])
            q = generic_quantize(d, cur)
            best = self.pick(q, picks[steps + 1], steps + 1)
            cur_q_ant = np.concatenate([q, [av[best]]])
            self.fus = f.update_sarsa(self.oa, self.fus, q_ant, r, cur_q_ant)
            states, q_ant = cur, cur_q_ant
            steps += 1
            total += r
            actions.append(best)
            if success == 1 or steps >= d["max_steps"]:
                break
        same = self.prev["R"] == f.R and self.prev["steps"] == steps and total > d["reward_good_above"] and self.prev["reward"] == total
        if same and not (np.abs(np.array(f.rconc[: f.R]) - self.prev["q"][: f.R]) >= d["qdiff_final_tolerance"]).any():
            self.converged = True
        self.prev["steps"], self.prev["reward"] = steps, total
        return actions, steps, total


EXPLORE = dict(epsilon=0.2, seed=4321, env_id_base=2 ** 32 - 5)      # the batch's global ids cross 2^32


def new_shape_case(nant, A, p=0, explore=None, override=None):
    """Description, environment, start states and the oracle mirrors of one new-shape case (no GPU needed).  override: fields of the
    description to replace (hyper-parameters: alpha, gamma, qdiff_pos, qdiff_neg, weight_thr, skip_rules)."""
    d = dict(point_desc(nant, A), **(override or {}))
    E, maxR = 16, 1024
    starts = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, (E, nant - 1)))
    base = explore["env_id_base"] if explore else 0
    return d, PointEnv(nant - 1), starts, [Mirror(d, starts[e], maxR, p=p, explore=explore, gid=base + e) for e in range(E)]


@pytest.mark.parametrize("nant", [2, 4, 6, 8])
@pytest.mark.parametrize("A", [3, 5, 11])
def test_new_shapes_follow_the_oracle(nant, A):
    follow_the_oracle(nant, A, 0)


@pytest.mark.parametrize("power", ["1", "2", "nant+1"])
@pytest.mark.parametrize("nant", [2, 5, 8])
@pytest.mark.parametrize("A", [3, 11])
def test_new_shapes_follow_the_oracle_at_other_powers(nant, A, power):
    """The same construct loops with agent.p = 1, 2 and nant + 1 (the learner's kernels without rule slices, run-time weight form)
    against mirrors built on ob.Five(..., p=p).  At most 10 % of an agent batch's picks may follow the device inside a tie of the
    oracle (1e-12 relative, Mirror.pick).  The oracle alone (a dry run of the mirrors on the CPU) has such near-ties at 32 to 55 of the
    617 to 2605 picks of a case, at most 7.6 % (nant 2, A 3, p 3): the two first picks of every agent (all Q = 0) and, at nant = 2,
    corner rules that learn action-independent values; the counts per case are in profiles/r08_shepard_power.md."""
    p = nant + 1 if power == "nant+1" else int(power)
    mirrors = follow_the_oracle(nant, A, p)
    ties, picks = sum(m.ties for m in mirrors), sum(m.picks for m in mirrors)
    assert ties * 10 <= picks, (ties, picks)


@pytest.mark.parametrize("nant", [2, 5, 8])
@pytest.mark.parametrize("A", [3, 11])
def test_new_shapes_explore_and_follow_the_oracle(nant, A):
    """The construct loops with epsilon = 0.2 on streams whose global ids cross 2^32: the mirrors take the picks of
    tests/explore_ref.py after the greedy pick.  The tie rule is the existing one (1e-12 relative, at most 10 % of a case's picks),
    taken over the picks that stayed greedy: only those can tie.  tests/test_explore_ref.py::test_new_shape_cases_explore_enough
    shows that every case has exploring picks that change the action."""
    mirrors = follow_the_oracle(nant, A, 0, explore=EXPLORE)
    ties, greedy_picks = sum(m.ties for m in mirrors), sum(m.picks - m.explored for m in mirrors)
    assert ties * 10 <= greedy_picks, (ties, greedy_picks)
    assert sum(m.changed for m in mirrors) >= 10


def follow_the_oracle(nant, A, p, explore=None, override=None, tol=1e-6):
    import torch
    d, env, starts, mirrors = new_shape_case(nant, A, p, explore=explore, override=override)
    E, maxR, episodes = 16, 1024, 4
    kw = dict(epsilon=explore["epsilon"], no_random=0, seed=explore["seed"], env_id_base=explore["env_id_base"]) if explore else {}
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV, p=p, **kw)
    assert agent.desc.p == p and mirrors[0].five.c.p == (p or nant)
    conv = frirl_amd.Convergence(prob, DEV)
    ss = torch.from_numpy(starts).to(DEV)
    for ep in range(episodes):
        _, aidx = frirl_amd.agent_begin(prob, agent, envs, ss)
        envs.done.copy_(torch.maximum(envs.done, conv.converged))          # converged agents sit the episode out (frirl_amd.train)
        chosen = [aidx.clone()]
        live = [(envs.done == 0).clone()]
        action = agent.grid_values[nant - 1][aidx.long()]
        for t in range(d["max_steps"]):
            obs, reward, success = env.step(torch, envs.states, action)
            nxt, nidx = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32))
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
            actions, steps, total = m.episode(env, [int(p[e]) for p in picks])
            got = [int(picks[t][e]) for t in range(len(actions))]
            assert got == actions, (nant, A, ep, e)
            assert int(envs.ep_steps[e]) == steps and float(envs.ep_reward[e]) == total and int(envs.done[e]) == 1
            R = m.five.R
            assert int(nrules[e]) == R, (nant, A, ep, e)
            assert (rant[e, :, :R] == np.array(m.five.rant[:R]).T).all()
            q, ref = rb[e, nant, :R], np.array(m.five.rconc[:R])
            assert (np.abs(q - ref) <= tol * np.maximum(np.abs(ref), 1e-9)).all()
            assert int(envs.fus[e]) == int(m.fus)
            assert int(conv.converged[e]) == int(m.converged), (nant, A, ep, e)
    return mirrors


# ---- 3. reset mask --------------------------------------------------------------------------------------------------------
def test_reset_mask_restarts_only_the_selected_rows():
    import torch
    nant, A, E = 4, 5, 64
    d = dict(point_desc(nant, A), max_steps=200)
    env = PointEnv(nant - 1)
    rng = np.random.default_rng(5)
    s0 = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    s1 = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.9, 0.9, (E, nant - 1)))).to(DEV)
    mask = torch.from_numpy(rng.uniform(size=E) < 0.4).to(DEV)
    runs = []
    for _ in range(3):                          # A: no reset, B: reset of the masked rows, C: every row restarted
        prob, agent, envs = frirl_amd.fresh_batch(d, E, 512, DEV)
        act, _ = frirl_amd.agent_begin(prob, agent, envs, s0)
        runs.append([prob, agent, envs, act])

    def step_all():
        for r in runs:
            prob, agent, envs, act = r
            obs, reward, success = env.step(torch, envs.states, act)
            nxt, _ = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32))
            r[3] = nxt

    for _ in range(9):
        step_all()
    b, c = runs[1], runs[2]
    act_b, _ = frirl_amd.agent_begin(b[0], b[1], b[2], s1, reset=mask.to(torch.uint8))
    b[3] = torch.where(mask, act_b, b[3])
    c[3], _ = frirl_amd.agent_begin(c[0], c[1], c[2], s1)
    keep, reset = ~mask, mask
    for t in range(12):
        sa, sb, sc = (state_arrays(r[0], r[2]) for r in runs)
        assert_same(sb, sa, ("kept", t), rows=keep)
        assert_same(sb, sc, ("reset", t), rows=reset)
        assert torch.equal(runs[1][2].episode[reset], torch.full_like(runs[1][2].episode[reset], 2))
        assert torch.equal(runs[1][2].episode[keep], torch.full_like(runs[1][2].episode[keep], 1))
        step_all()


# ---- 4. scale -------------------------------------------------------------------------------------------------------------
def test_65536_agents_with_filling_rule_bases():
    import torch
    nant, A, E = 6, 11, 65536
    d = dict(point_desc(nant, A), max_steps=60)
    env = PointEnv(nant - 1)
    maxR = 2 ** nant + 16
    prob, agent, envs = frirl_amd.fresh_batch(d, E, maxR, DEV)
    starts = (torch.rand((E, nant - 1), generator=torch.Generator(device=DEV).manual_seed(3), device=DEV, dtype=torch.float64) * 1.8 - 0.9)
    act, _ = frirl_amd.agent_begin(prob, agent, envs, starts)
    episodes = torch.zeros((E,), dtype=torch.int32, device=DEV)
    for it in range(300):
        restart = envs.done != 0
        nact, _ = frirl_amd.agent_begin(prob, agent, envs, starts, reset=restart.to(torch.uint8))
        act = torch.where(restart, nact, act)
        episodes += restart.to(torch.int32)
        obs, reward, success = env.step(torch, envs.states, act)
        act, _ = frirl_amd.agent_observe(prob, agent, envs, obs.contiguous(), reward.contiguous(), success.to(torch.int32))
    torch.cuda.synchronize()
    done, steps, status, nrules = envs.done, envs.ep_steps, envs.status, prob.nrules
    success = success.to(torch.int32)
    assert bool(((done == 0) | (done == 1)).all()) and bool((steps >= 1).all()) and bool((steps <= d["max_steps"]).all())
    assert torch.equal(done, ((success == 1) | (steps >= d["max_steps"])).to(torch.int32))       # every row stepped in the last call
    assert bool(((status >= frirl_amd.UPD_EXACT) & (status <= frirl_amd.UPD_FULL)).all())
    assert bool((nrules <= maxR).all()) and bool((nrules >= 2 ** nant).all())
    full = status == frirl_amd.UPD_FULL
    assert bool((nrules[full] == maxR).all()) and int((nrules == maxR).sum()) > 0
    assert torch.equal(envs.episode, episodes + 1) and int(episodes.min()) >= 300 // d["max_steps"] - 1
