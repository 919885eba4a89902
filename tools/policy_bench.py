#!/usr/bin/env python3
"""Caller-stepped shared-rule-base numbers (frirl_hip_policy_observe, reduce_external) next to the in-kernel forms:
  (a) us per frirl_hip_policy_observe call on the oracle-trained acrobot rule base (367 rules), Q = 1023 and 65 536, per lane-group
      shape (options policy_group / policy_slices) and for the shipped selection; beside it frirl_hip_rollout_shared's time per step for
      the same start states (call time / steps of the longest episode).  The observe calls replay recorded environment data, so only
      the launch is timed (hip events around N back-to-back calls, rows kept live by a large max_steps).
  (b) wall time of the three demo reductions through reduce_external (frirl_hip_env_step as the caller's environment), through
      frirl_hip_reduce_shared, and of the oracle's sequential loop on one host core; strategy 1.
python tools/policy_bench.py [--reps 200]
With --agents E instead: the reduction of E rule bases learned on the device (start states spread +-10 %, as tools/reduce_bench.py
--agents) in the caller's environment, strategy 1, frirl_hip_env_step as the environment, mountaincar and acrobot:
  reduce_external_batch (one launch per step for all agents)  against  a loop of reduce_external over the same rule bases,
  and Problem.reduce_batch (the environment inside the kernel) as the floor.
Host clock around calls that end in a synchronise, rule bases restored outside the window, one warm-up, the sides alternating:
python tools/policy_bench.py --agents 64 [--timed 2] [--loop-sample 64] [--only mountaincar]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
import frirl_amd
from oracle import binding as ob


def oracle_trained(env):
    fr = ob.Frirl(env, trig_mode=1)
    assert fr.run() == 1
    return fr


def shared_problem(fr, dev):
    f = fr.five
    R, nant = f.R, f.nant
    maxR = R + 8 + (R & 1)
    rb = np.zeros((1, nant + 1, maxR))
    rb[0, :nant, :R] = f.veval[:, :R]
    rb[0, nant, :R] = f.rconc[:R]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return frirl_amd.Problem(t(np.array(f.u)), t(np.array(f.ve)), t(rb), t(np.array([R], dtype=np.int32)))


def observe_us(prob, agent, Q, shape, reps, dev):
    d = frirl_amd.demo_describe("acrobot")
    ns = prob.nant - 1
    g = torch.Generator(device=dev); g.manual_seed(7)
    lo = torch.tensor([d["grids"][k].min() for k in range(ns)], dtype=torch.float64, device=dev)
    hi = torch.tensor([d["grids"][k].max() for k in range(ns)], dtype=torch.float64, device=dev)
    s = (lo + torch.rand((Q, ns), dtype=torch.float64, device=dev, generator=g) * (hi - lo)).contiguous()
    old = (frirl_amd.set_option("policy_group", shape[0]), frirl_amd.set_option("policy_slices", shape[1]))
    try:
        rows = frirl_amd.PolicyRows(Q, dev)
        action, _ = prob.policy_begin(agent, rows, s)
        obs, reward, success, _ = frirl_amd.env_step(agent, action, s)
        success.zero_()                                    # rows stay live: every call does the full work
        io, _, _ = frirl_amd._agent_io(prob, obs, None, reward, success, E=Q)
        import ctypes as C
        call = lambda: frirl_amd.lib().frirl_hip_policy_observe(C.byref(prob.tables), C.byref(prob._bases), C.byref(agent.desc), C.byref(rows.desc),
                                                                C.byref(io), frirl_amd._stream())
        for _ in range(20):
            assert call() == 0
        torch.cuda.synchronize()
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / reps
            best = us if best is None else min(best, us)
        return best
    finally:
        frirl_amd.set_option("policy_group", old[0])
        frirl_amd.set_option("policy_slices", old[1])


def agents_leg(env, E, a, dev):
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

    def step_fn(states, action):
        obs, reward, success, q = frirl_amd.env_step(agent, action, states)
        return (obs, reward, success, q) if env == "cartpole" else (obs, reward, success)

    sample = list(range(E)) if a.loop_sample >= E else [int(i) for i in np.linspace(0, E - 1, a.loop_sample).astype(int)]
    views = [frirl_amd.Problem(prob.u, prob.ve, prob.rb[e:e + 1], prob.nrules[e:e + 1], prob.uidx[e:e + 1]) for e in sample]
    depth = frirl_amd.lib().frirl_hip_reduce_batch_depth(E, d["A"])
    out = {"what": "reduce_agents", "env": env, "agents": E, "converged": int((run.conv.converged == 1).sum()), "rules_before_sum": int(snap[1].sum()),
           "depth": depth, "loop_depth": 10, "loop_agents_timed": len(sample), "stepped_batch_s": [], "stepped_loop_s": [], "in_kernel_batch_s": []}
    for rep in range(a.timed + 1):                                   # rep 0 warms every side up
        restore()
        t0 = time.perf_counter()
        kept, res = frirl_amd.reduce_external_batch(prob, agent, lambda Q, n: ss.repeat_interleave(n, 0), step_fn, 1, 0.0, 0, rant=envs.rant)
        torch.cuda.synchronize()
        dt_b = time.perf_counter() - t0
        after_b = np.array([r.rules_after for r in res])
        steps_sum = int(sum(r.steps_incremental for r in res))
        restore()
        after_l = []
        t0 = time.perf_counter()
        for e, view in zip(sample, views):
            st = ss[e]
            _, r1 = frirl_amd.reduce_external(view, agent, lambda Q: st.expand(Q, ns).contiguous(), step_fn, 1, 0.0, 0, rant=envs.rant[e])
            after_l.append(r1.rules_after)
        torch.cuda.synchronize()
        dt_l = time.perf_counter() - t0
        restore()
        t0 = time.perf_counter()
        _, res_k = prob.reduce_batch(agent, 1, 0.0, 0, rant=envs.rant, start_states=ss)
        torch.cuda.synchronize()
        dt_k = time.perf_counter() - t0
        assert (after_b[sample] == np.array(after_l)).all(), "batched and single-base stepped reductions disagree"
        assert (after_b == np.array([r.rules_after for r in res_k])).all(), "stepped and in-kernel batched reductions disagree"
        if rep:
            out["stepped_batch_s"].append(round(dt_b, 4))
            out["stepped_loop_s"].append(round(dt_l, 4))
            out["in_kernel_batch_s"].append(round(dt_k, 4))
    scale = E / len(sample)
    out["stepped_loop_s_all_agents"] = [round(x * scale, 4) for x in out["stepped_loop_s"]]
    out["loop_extrapolated"] = len(sample) < E
    out.update(rules_after_sum=int(after_b.sum()), rounds_max=max(r.rounds for r in res), baseline_steps_sum=steps_sum,
               loop_over_batch_min_over_min=round(min(out["stepped_loop_s_all_agents"]) / min(out["stepped_batch_s"]), 2),
               batch_over_in_kernel_min_over_min=round(min(out["stepped_batch_s"]) / min(out["in_kernel_batch_s"]), 2))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--agents", type=int, default=0)
    ap.add_argument("--timed", type=int, default=2)
    ap.add_argument("--loop-sample", type=int, default=64)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.agents:
        for env in ([a.only] if a.only else ["mountaincar", "acrobot"]):
            agents_leg(env, a.agents, a, dev)
        return
    fr = oracle_trained("acrobot")
    prob = shared_problem(fr, dev)
    agent = frirl_amd.demo_agent(frirl_amd.demo_describe("acrobot"), dev, max_steps=1 << 30)
    for Q in (1023, 65536):
        for shape in ((0, 0), (1, 1), (4, 1), (4, 4), (4, 8)):
            print(json.dumps({"what": "policy_observe", "rules": fr.five.R, "Q": Q, "group": shape[0], "slices": shape[1],
                              "us_per_call": round(observe_us(prob, agent, Q, shape, a.reps, dev), 2)}), flush=True)
        ag = frirl_amd.demo_agent(frirl_amd.demo_describe("acrobot"), dev)
        ss = torch.from_numpy(np.tile(np.array([fr.dim(k)["values_def"] for k in range(fr.nstates)]), (Q, 1))).to(dev)
        best = None
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps, _, _, _ = prob.rollout_shared(ag, Q, start_states=ss)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or rep == 0 else min(best, dt)
        print(json.dumps({"what": "rollout_shared", "Q": Q, "longest_episode": int(steps.max()), "call_s": round(best, 5),
                          "us_per_step": round(best * 1e6 / int(steps.max()), 2)}), flush=True)
    for env in ("mountaincar", "acrobot", "cartpole"):
        fr = oracle_trained(env)
        agent = frirl_amd.demo_agent(frirl_amd.demo_describe(env), dev)
        ns = fr.nstates
        start = torch.from_numpy(np.array([fr.dim(k)["values_def"] for k in range(ns)])).to(dev)

        def step_fn(states, action):
            obs, reward, success, q = frirl_amd.env_step(agent, action, states)
            return (obs, reward, success, q) if env == "cartpole" else (obs, reward, success)

        out = {"what": "reduce", "env": env, "rules_before": fr.five.R}
        for name in ("external", "in_kernel"):
            best = None
            for rep in range(2):
                p = shared_problem(fr, dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "external":
                    kept, res = frirl_amd.reduce_external(p, agent, lambda Q: start.expand(Q, ns).contiguous(), step_fn, 1)
                else:
                    kept, res = p.reduce_shared(agent, 1)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            out[name + "_s"] = round(best, 4)
            out[name + "_rules_after"] = res.rules_after
            out["steps_incremental"], out["rounds"] = res.steps_incremental, res.rounds
        t0 = time.perf_counter()
        fr.reduce(1, 0.0)
        out["oracle_sequential_s"] = round(time.perf_counter() - t0, 4)
        out["oracle_rules_after"] = fr.five.R
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
