#!/usr/bin/env python3
"""What the expected-SARSA flag costs the users of the EXPECT learner kernels (level 4 of the launch table, learn_*_4.hip), measured against
the TARGET kernels on identical inputs, and a record of how the three targets learn.
   python tools/expect_bench.py [--env mountaincar --env acrobot] [--agents 65536 --agents 4096] [--rounds 5] [--max-episodes 400]
                                [--quality-agents 4096] [--quality-episodes 60] [--out FILE]
cost     E agents of a demo, one start state each on the state grid (the workload of tools/target_bench.py), exploration rows set: 16
         (epsilon, horizon) sets, epsilon 0.05 / 0.1 / 0.2 / 0.3 x horizon 2 / 4 / 8 / 16, agent e under set e mod 16.  Sides,
         alternating in one process, a fresh batch before each (outside the timed window), round 0 warms up, `rounds` timed rounds:
           t  frirl_hip_learn_train_target, an all-SARSA column                         the yardstick: its code is the parent's, unchanged
           z  frirl_hip_learn_train_expect, the same column and an all-zero flag column  the EXPECT kernels doing the same work, bit for bit
           x  frirl_hip_learn_train_expect, every agent flagged                         another trajectory: other steps, other rule counts
         Timed with device events around the call.  Per side: every round, the mean and the spread (max - min) of its own rounds.
quality  a constant epsilon = 0.1 population through the batch object (frirl_hip_batch_set_exploration, _set_target or _set_expected,
         frirl_hip_batch_train), then frirl_hip_batch_evaluate from every agent's own start: successes under SARSA, Q and expected SARSA
         after the same number of episodes.  A record, no claim: one seed, one run.
One JSON line per cell; --out appends them to a file as well."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
import frirl_amd

NSETS, MAXR, SEED = 16, 1024, 1265
SETS = [(eps, h) for eps in (0.05, 0.1, 0.2, 0.3) for h in (2, 4, 8, 16)]


def cost(env, E, a, dev):
    d = frirl_amd.demo_describe(env)
    g = torch.Generator(device=dev).manual_seed(1)
    start = torch.stack([torch.from_numpy(d["grids"][k]).to(dev)[torch.randint(0, len(d["grids"][k]), (E,), generator=g, device=dev)]
                         for k in range(d["nstates"])], 1).contiguous()
    explore = frirl_amd.ExploreRows(E, dev, epsilon=np.array([SETS[e % NSETS][0] for e in range(E)]),
                                    horizon=np.array([SETS[e % NSETS][1] for e in range(E)], dtype=np.int32))
    target = frirl_amd.TargetRows(E, dev, target=np.zeros(E, dtype=np.uint8))
    sides = dict(t=None, z=frirl_amd.ExpectRows(E, dev, expected=np.zeros(E, dtype=np.uint8)), x=frirl_amd.ExpectRows(E, dev, expected=np.ones(E, dtype=np.uint8)))
    times = {k: [] for k in sides}
    last = {}
    for rnd in range(a.rounds + 1):                     # round 0 warms up every kernel variant the timed rounds launch
        for k, expect in sides.items():
            prob, agent, envs = frirl_amd.fresh_batch(d, E, MAXR, dev, start_states=start, no_random=0, seed=SEED)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = frirl_amd.train_persistent(prob, agent, envs, max_episodes=a.max_episodes, budget=a.budget, explore=explore, target=target, expect=expect)
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                times[k].append(t0.elapsed_time(t1) / 1e3)
            last[k] = dict(steps=r.steps_total.clone(), nrules=prob.nrules.clone(), rb=prob.rb.clone(), converged=int(r.conv.converged.sum()), launches=r.launches)
    out = dict(mode="cost", env=env, agents=E, budget=a.budget, max_episodes=a.max_episodes, rounds=a.rounds)
    for k in sides:
        t = np.array(times[k])
        out[k] = dict(s=[round(float(v), 4) for v in t], mean=float(t.mean()), spread=float(t.max() - t.min()), env_steps=int(last[k]["steps"].sum()),
                      converged=last[k]["converged"], mean_rules=float(last[k]["nrules"].float().mean()), launches=last[k]["launches"])
    out["z_over_t"] = out["z"]["mean"] / out["t"]["mean"]
    out["x_over_t"] = out["x"]["mean"] / out["t"]["mean"]
    out["z_minus_t_over_t_spread"] = (out["z"]["mean"] - out["t"]["mean"]) / max(out["t"]["spread"], 1e-12)
    out["z_equals_t_bit_for_bit"] = bool(torch.equal(last["z"]["rb"], last["t"]["rb"]) and torch.equal(last["z"]["steps"], last["t"]["steps"]))
    return out


def quality(env, E, a):
    lib = frirl_amd.lib()
    d = frirl_amd.demo_describe(env)
    rng = np.random.default_rng(3)
    start = np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))
    out = dict(mode="quality", env=env, agents=E, epsilon=0.1, episodes=a.quality_episodes)
    for name in ("sarsa", "q", "expected"):
        batch = frirl_amd.demo_batch_object(env, E, MAXR, start_states=start, seed=SEED)
        try:
            frirl_amd.batch_set_exploration(batch, epsilon=np.full(E, 0.1))
            if name == "expected":
                frirl_amd.batch_set_expected(batch, None, 1)
            else:
                frirl_amd.batch_set_target(batch, None, frirl_amd.TARGET_Q if name == "q" else frirl_amd.TARGET_SARSA)
            frirl_amd.check(lib.frirl_hip_batch_train(batch, a.quality_episodes + 1, None), "frirl_hip_batch_train")
            scores, best = (frirl_amd.RolloutScore * E)(), C.c_int32(0)
            frirl_amd.check(lib.frirl_hip_batch_evaluate(batch, 1, None, scores, C.byref(best)), "frirl_hip_batch_evaluate")
            rep = frirl_amd.batch_agent_report(batch)
            out[name] = dict(successes=int(sum(s.successes for s in scores)), mean_reward=float(np.mean([s.reward_sum for s in scores])),
                             mean_rules=float(rep["rules"].mean()), converged=int(rep["converged"].sum()))
        finally:
            lib.frirl_hip_batch_destroy(batch)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", action="append")
    ap.add_argument("--agents", action="append", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=4096)
    ap.add_argument("--max-episodes", type=int, default=400)
    ap.add_argument("--quality-agents", type=int, default=4096)
    ap.add_argument("--quality-episodes", type=int, default=60)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cells = []
    for env in a.env or ["mountaincar", "acrobot"]:
        for E in a.agents or [65536, 4096]:
            assert E % NSETS == 0
            cells.append(cost(env, E, a, dev))
            print(json.dumps(cells[-1]), flush=True)
        if a.quality_agents > 0:
            cells.append(quality(env, a.quality_agents, a))
            print(json.dumps(cells[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for c in cells:
                f.write(json.dumps(c) + "\n")


if __name__ == "__main__":
    main()
