#!/usr/bin/env python3
"""Evaluation-mode numbers on the three demo rule bases (learned here on the GPU, E = 1):
  * wall time of the speculative try-remove reduction (frirl_hip_reduce_shared), strategies 1 and 2
  * throughput of greedy roll-outs on the shared rule base (frirl_hip_rollout_shared), Q environments
python tools/reduce_bench.py [--depth 10] [--envs 65536]
With --agents E (repeatable) instead: the batched reduction of E learned rule bases (frirl_hip_reduce_batch, every agent from its own
start state) against a loop of frirl_hip_reduce_shared over the same rule bases with values_def set per agent, mountaincar and acrobot:
python tools/reduce_bench.py --agents 64 --agents 4096 [--depth 0] [--loop-sample 64] [--reps 2]
With --agents E --starts K (both repeatable): the reduction against K start states per agent (frirl_hip_reduce_batch_starts, strategy 1) on
the same learned rule bases: n = 1 against frirl_hip_reduce_batch (alternating), n = K against n = 1 (time, rounds, rules kept), and how many
of the independent test starts that the un-reduced rule bases solve are still solved afterwards (Problem.rollout_batch):
python tools/reduce_bench.py --agents 64 --starts 4 --starts 16 [--reps 3] [--spread 0.1] [--test-starts 32]
With --stepped in addition: the same inputs through the caller-stepped reducers, the demo dynamics stepped from torch (frirl_hip_env_step):
n = 1 made with start states against the reducer made without (reduce_external_batch, alternating), n = K stepped against the in-kernel
frirl_hip_reduce_batch_starts, and the share of the staged workgroups' rows that are holes with drop_bad_starts = 1:
python tools/reduce_bench.py --agents 64 --starts 16 --stepped [--reps 3]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
import frirl_amd


def learned(env, dev):
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, 1, 1024, dev)
    conv = frirl_amd.train(prob, agent, envs)
    torch.cuda.synchronize()
    assert int(conv.converged[0]) == 1
    return prob, agent, envs


def batch_leg(env, E, a, dev):
    """Host clock around calls that end in a device synchronise (both entry points synchronise before they return); the two sides
    alternate, rule bases restored from a snapshot before every timed call (outside the window); first repetition = warm-up."""
    d = frirl_amd.demo_describe(env)
    ns = d["nstates"]
    rng = np.random.default_rng(11)
    start = np.zeros((E, ns))
    for k in range(ns):
        g = d["grids"][k]
        start[:, k] = np.clip(d["values_def"][k] + rng.uniform(-0.1, 0.1, E) * (g.max() - g.min()), g.min(), g.max())
        start[0, k] = d["values_def"][k]
    ss = torch.from_numpy(np.ascontiguousarray(start)).to(dev)
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 512, dev, start_states=ss)
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=400)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (prob.rb, prob.nrules, prob.uidx, envs.rant)]

    def restore():
        for t, t0 in zip((prob.rb, prob.nrules, prob.uidx, envs.rant), snap):
            t.copy_(t0)
        torch.cuda.synchronize()

    nr0 = snap[1].cpu().numpy()
    depth = a.depth or frirl_amd.lib().frirl_hip_reduce_batch_depth(E, d["A"])
    # the loop's side: one-base views of the same slabs, built outside the timed window; all agents, or an evenly spaced sample
    # (--loop-sample 0: the batched side alone, for depth sweeps)
    sample = list(range(E)) if 0 < a.loop_sample >= E else [int(i) for i in np.linspace(0, E - 1, a.loop_sample).astype(int)]
    views = [frirl_amd.Problem(prob.u, prob.ve, prob.rb[e:e + 1], prob.nrules[e:e + 1], prob.uidx[e:e + 1]) for e in sample]
    out = {"env": env, "agents": E, "converged": int((run.conv.converged == 1).sum()), "rules_before_sum": int(nr0.sum()), "depth": depth,
           "loop_depth": a.depth or 10, "loop_agents_timed": len(sample), "batch_s": [], "loop_s": []}
    for strategy in (1,):
        for rep in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            kept, res = prob.reduce_batch(agent, strategy, 0.0, a.depth, rant=envs.rant, start_states=ss)
            dt_b = time.perf_counter() - t0
            after_b = np.array([r.rules_after for r in res])
            restore()
            after_l = []
            t0 = time.perf_counter()
            for e, view in zip(sample, views):
                for k in range(ns):
                    agent.desc.values_def[k] = float(start[e, k])
                _, r1 = view.reduce_shared(agent, strategy, 0.0, a.depth, rant=envs.rant[e])
                after_l.append(r1.rules_after)
            dt_l = time.perf_counter() - t0
            for k in range(ns):
                agent.desc.values_def[k] = float(d["values_def"][k])
            assert (after_b[sample] == np.array(after_l)).all(), "batched and single-base reductions disagree"
            if rep:                                                  # rep 0 warms both sides up
                out["batch_s"].append(round(dt_b, 4))
                if sample:
                    out["loop_s"].append(round(dt_l, 4))
        out.update(strategy=strategy, rules_after_sum=int(after_b.sum()), rounds_max=max(r.rounds for r in res), rollouts_sum=int(sum(r.rollouts for r in res)))
    if sample:
        scale = E / len(sample)
        out["loop_s_all_agents"] = [round(x * scale, 4) for x in out["loop_s"]]
        out["loop_extrapolated"] = len(sample) < E
        out["speedup_min_over_min"] = round(min(out["loop_s_all_agents"]) / min(out["batch_s"]), 2)
    else:
        del out["loop_s"], out["loop_depth"]
    print(json.dumps(out), flush=True)


def starts_inputs(env, E, a, dev):
    """What starts_leg and stepped_leg share: the rule bases of batch_leg (trained from starts at +-0.1 span), restore() to put them
    back, the validation starts val [E, max K, ns] (row 0 = the agent's own start, rows 1.. = own +- spread * span, seed 17) and
    around(n, seed) for further draws."""
    d = frirl_amd.demo_describe(env)
    ns = d["nstates"]
    lo = np.array([d["grids"][k].min() for k in range(ns)])
    hi = np.array([d["grids"][k].max() for k in range(ns)])
    vd = np.array([d["values_def"][k] for k in range(ns)])
    rng = np.random.default_rng(11)
    start = np.zeros((E, ns))
    for k in range(ns):
        start[:, k] = np.clip(vd[k] + rng.uniform(-0.1, 0.1, E) * (hi[k] - lo[k]), lo[k], hi[k])
        start[0, k] = vd[k]
    tens = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ss = tens(start)
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 512, dev, start_states=ss)
    run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=400)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (prob.rb, prob.nrules, prob.uidx, envs.rant)]

    def restore():
        for t, t0 in zip((prob.rb, prob.nrules, prob.uidx, envs.rant), snap):
            t.copy_(t0)
        torch.cuda.synchronize()

    def around(n, seed):
        r = np.random.default_rng(seed)
        x = np.clip(start[:, None, :] + r.uniform(-a.spread, a.spread, (E, n, ns)) * (hi - lo), lo, hi)
        return x

    Kmax = max(a.starts)
    val = around(Kmax, 17)
    val[:, 0, :] = start
    return d, prob, agent, envs, run, snap, restore, tens, ss, val, around


def starts_leg(env, E, a, dev):
    """Test starts: --test-starts per agent, spread as the validation starts, seed 5.  Host clock around calls that end in a device
    synchronise; rule bases restored from a snapshot before every timed call; first repetition = warm-up."""
    d, prob, agent, envs, run, snap, restore, tens, ss, val, around = starts_inputs(env, E, a, dev)
    ns = d["nstates"]
    test = tens(around(a.test_starts, 5).reshape(E * a.test_starts, ns))

    def solved():
        _, reward, _, _ = prob.rollout_batch(agent, a.test_starts, start_states=test)
        torch.cuda.synchronize()
        return (reward > d["reward_good_above"]).cpu().numpy()

    base = solved()
    out = {"env": env, "agents": E, "converged": int((run.conv.converged == 1).sum()), "rules_before_sum": int(snap[1].sum()), "strategy": 1,
           "spread": a.spread, "test_starts": int(base.size), "test_solved_before": int(base.sum())}
    # 1. n = 1 against frirl_hip_reduce_batch, alternating
    one = tens(val[:, :1, :])
    t_b, t_s = [], []
    for rep in range(max(a.reps, 3) + 1):
        restore()
        t0 = time.perf_counter()
        kept_b, res_b = prob.reduce_batch(agent, 1, 0.0, a.depth, rant=envs.rant, start_states=ss)
        dt_b = time.perf_counter() - t0
        restore()
        t0 = time.perf_counter()
        kept_s, res_s, _ = prob.reduce_batch_starts(agent, 1, 0.0, a.depth, one, rant=envs.rant)
        dt_s = time.perf_counter() - t0
        assert all((x == y).all() for x, y in zip(kept_b, kept_s)) and [r.rollouts for r in res_b] == [r.rollouts for r in res_s]
        if rep:
            t_b.append(round(dt_b, 4)); t_s.append(round(dt_s, 4))
    lost1 = base & ~solved()                                          # the state after the last n = 1 run
    out.update(reduce_batch_s=t_b, starts_n1_s=t_s, n1_over_reduce_batch_min=round(min(t_s) / min(t_b), 3),
               n1_over_reduce_batch_median=round(float(np.median(t_s) / np.median(t_b)), 3),
               n1={"rules_after_sum": int(sum(r.rules_after for r in res_s)), "rounds_max": max(r.rounds for r in res_s),
                   "depth": a.depth or frirl_amd.lib().frirl_hip_reduce_batch_starts_depth(E, d["A"], 1), "test_lost": int(lost1.sum())})
    # 2. n = K, start states whose baseline is not good left out
    for K in a.starts:
        vk = tens(val[:, :K, :])
        ts = []
        for rep in range(max(a.reps, 3) + 1):
            restore()
            t0 = time.perf_counter()
            _, res, per = prob.reduce_batch_starts(agent, 1, 0.0, a.depth, vk, drop_bad_starts=True, rant=envs.rant)
            dt = time.perf_counter() - t0
            if rep:
                ts.append(round(dt, 4))
        lost = base & ~solved()
        out[f"n{K}"] = {"s": ts, "over_n1_min": round(min(ts) / min(t_s), 2), "rules_after_sum": int(sum(r.rules_after for r in res)),
                        "rounds_max": max(r.rounds for r in res), "rollouts_sum": int(sum(r.rollouts for r in res)),
                        "depth": a.depth or frirl_amd.lib().frirl_hip_reduce_batch_starts_depth(E, d["A"], K),
                        "starts_used": int(sum(p.used for row in per for p in row)), "starts_given": E * K, "test_lost": int(lost.sum()),
                        "lost_coverage_recovered": round(1.0 - lost.sum() / lost1.sum(), 3) if lost1.sum() else None}
    print(json.dumps(out), flush=True)


def stepped_leg(env, E, a, dev):
    """The inputs of starts_leg through the caller-stepped reducers; every environment step is one frirl_hip_env_step over all rows of
    the round and one observe.  Clock and repetitions as starts_leg.  Rows per workgroup for the hole share: 256 / (G * 8), the shape
    the depth rule keeps resident (G = 4 lanes per row for up to 4 actions, else 8)."""
    d, prob, agent, envs, run, snap, restore, tens, ss, val, around = starts_inputs(env, E, a, dev)

    def step_fn(states, action):
        obs, reward, success, q = frirl_amd.env_step(agent, action, states)
        return (obs, reward, success, q) if env == "cartpole" else (obs, reward, success)

    def rows_of(S):
        def reset_fn(Q, rpa, n):
            q = torch.arange(Q, device=dev)
            return S[q // rpa, q % n].contiguous()
        return reset_fn

    def timed(fn):
        restore()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out = {"env": env, "agents": E, "converged": int((run.conv.converged == 1).sum()), "rules_before_sum": int(snap[1].sum()), "strategy": 1,
           "spread": a.spread, "stepped": True}
    # (a) n = 1: the reducer made with start states against the one made without, alternating
    one = tens(val[:, :1, :])
    t_p, t_s = [], []
    for rep in range(max(a.reps, 3) + 1):
        dt_p, (kept_p, res_p) = timed(lambda: frirl_amd.reduce_external_batch(prob, agent, lambda Q, n: ss.repeat_interleave(n, 0), step_fn, 1, 0.0, a.depth,
                                                                             rant=envs.rant))
        dt_s, (kept_s, res_s, _) = timed(lambda: frirl_amd.reduce_external_batch_starts(prob, agent, rows_of(one), step_fn, 1, 1, 0.0, a.depth, rant=envs.rant))
        assert all((x == y).all() for x, y in zip(kept_p, kept_s)) and [r.rollouts for r in res_p] == [r.rollouts for r in res_s]
        if rep:
            t_p.append(round(dt_p, 4)); t_s.append(round(dt_s, 4))
    out.update(plain_reducer_s=t_p, starts_reducer_n1_s=t_s, n1_over_plain_min=round(min(t_s) / min(t_p), 3),
               n1_over_plain_median=round(float(np.median(t_s) / np.median(t_p)), 3), rules_after_sum_n1=int(sum(r.rules_after for r in res_s)))
    # (b) n = K with drop_bad_starts = 1: stepped against in-kernel; (c) the holes of the stepped rows
    for K in a.starts:
        vk = tens(val[:, :K, :])
        t_k, t_x = [], []
        for rep in range(max(a.reps, 3) + 1):
            dt_k, (kept_k, res_k, _) = timed(lambda: prob.reduce_batch_starts(agent, 1, 0.0, a.depth, vk, drop_bad_starts=True, rant=envs.rant))
            dt_x, (kept_x, res_x, per_x) = timed(lambda: frirl_amd.reduce_external_batch_starts(prob, agent, rows_of(vk), step_fn, 1, K, 0.0, a.depth,
                                                                                                 rant=envs.rant, drop_bad_starts=True))
            same = sum(len(x) == len(y) and (x == y).all() for x, y in zip(kept_k, kept_x))
            if rep:
                t_k.append(round(dt_k, 4)); t_x.append(round(dt_x, 4))
        # one more run, not timed: rows that exist after every begin, in workgroups of `epb` rows of one agent
        restore()
        epb = 256 // ((4 if d["A"] <= 4 else 8) * 8)
        lanes = rows = steps = 0
        red = frirl_amd.BatchReducer(prob, agent, 1, 0.0, a.depth, envs.rant, starts=K, drop_bad_starts=True)
        try:
            rnd = 0
            while red.next_round() > 0:
                states = rows_of(vk)(red.Q, red.rows_per_agent, K)
                action, _ = red.begin(states)
                if rnd:
                    ex = (red.row_done() == 0).view(E, red.rows_per_agent)
                    pad = (-red.rows_per_agent) % epb
                    wg = torch.nn.functional.pad(ex, (0, pad)).view(E, -1, epb)
                    lanes += int(wg.any(2).sum()) * epb
                    rows += int(ex.sum())
                live = red.Q
                while live > 0:
                    o = step_fn(states, action)
                    action, _, live = red.observe(o[0].contiguous(), o[1].contiguous(), o[2].to(torch.int32).contiguous(),
                                                  q_obs=o[3].contiguous() if len(o) > 3 else None)
                    states = o[0]
                    steps += 1
                red.end_round()
                rnd += 1
        finally:
            red.close()
        out[f"n{K}"] = {"in_kernel_s": t_k, "stepped_s": t_x, "stepped_over_in_kernel_min": round(min(t_x) / min(t_k), 2),
                        "agents_with_equal_kept": int(same), "rules_after_sum": int(sum(r.rules_after for r in res_x)),
                        "rounds_max": max(r.rounds for r in res_x), "rollouts_sum": int(sum(r.rollouts for r in res_x)),
                        "depth": a.depth or frirl_amd.lib().frirl_hip_reduce_batch_starts_depth(E, d["A"], K), "observe_calls": steps,
                        "starts_used": int(sum(p.used for row in per_x for p in row)), "starts_given": E * K, "rows_per_workgroup": epb,
                        "rows_in_staged_workgroups": lanes, "rows_that_exist": rows, "share_lost_to_holes": round(1.0 - rows / lanes, 4) if lanes else None}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--agents", type=int, action="append", default=[])
    ap.add_argument("--loop-sample", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--starts", type=int, action="append", default=[])
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--test-starts", type=int, default=32)
    ap.add_argument("--stepped", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.agents:
        for env in ([a.only] if a.only else ["mountaincar", "acrobot"]):
            for E in a.agents:
                (stepped_leg if a.stepped and a.starts else starts_leg if a.starts else batch_leg)(env, E, a, dev)
        return
    for env in ("mountaincar", "cartpole", "acrobot"):
        prob, agent, envs = learned(env, dev)
        R = int(prob.nrules[0])
        rb0, nr0 = prob.rb.clone(), prob.nrules.clone()
        ui0 = prob.uidx.clone() if prob.uidx is not None else None
        # roll-outs from perturbed start states
        ns = prob.nant - 1
        g = torch.Generator(device=dev); g.manual_seed(3)
        d = frirl_amd.demo_describe(env)
        lo = torch.tensor([d["grids"][k].min() for k in range(ns)], dtype=torch.float64, device=dev)
        hi = torch.tensor([d["grids"][k].max() for k in range(ns)], dtype=torch.float64, device=dev)
        vd = torch.tensor([d["values_def"][k] for k in range(ns)], dtype=torch.float64, device=dev)
        ss = (vd + (torch.rand((a.envs, ns), dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.2 * (hi - lo)).clamp(lo, hi).contiguous()
        prob.rollout_shared(agent, a.envs, start_states=ss)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps, reward, success, _ = prob.rollout_shared(agent, a.envs, start_states=ss)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tot = int(steps.sum())
        print(json.dumps({"env": env, "rules": R, "rollouts": a.envs, "env_steps": tot, "s": round(dt, 4), "env_steps_per_s": tot / dt,
                          "success_frac": float((success == 1).double().mean())}))
        for strategy in (1, 2):
            best = None
            for rep in range(3):
                prob.rb.copy_(rb0); prob.nrules.copy_(nr0)
                if ui0 is not None:
                    prob.uidx.copy_(ui0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kept, res = prob.reduce_shared(agent, strategy, 0.0, a.depth)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            print(json.dumps({"env": env, "strategy": strategy, "rules_before": R, "rules_after": res.rules_after, "launches": res.rounds,
                              "rollouts": res.rollouts, "steps_incremental": res.steps_incremental, "gpu_s": round(best, 4)}))


if __name__ == "__main__":
    main()
