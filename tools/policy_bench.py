#!/usr/bin/env python3
"""Caller-stepped shared-rule-base numbers (frirl_hip_policy_observe, reduce_external) next to the in-kernel forms:
  (a) us per frirl_hip_policy_observe call on the oracle-trained acrobot rule base (367 rules), Q = 1023 and 65 536, per lane-group
      shape (options policy_group / policy_slices) and for the shipped selection; beside it frirl_hip_rollout_shared's time per step for
      the same start states (call time / steps of the longest episode).  The observe calls replay recorded environment data, so only
      the launch is timed (hip events around N back-to-back calls, rows kept live by a large max_steps).
  (b) wall time of the three demo reductions through reduce_external (frirl_hip_env_step as the caller's environment), through
      frirl_hip_reduce_shared, and of the oracle's sequential loop on one host core; strategy 1.
python tools/policy_bench.py [--reps 200]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
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
