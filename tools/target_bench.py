#!/usr/bin/env python3
"""What the TD-target byte costs the users of the TARGET learner kernels (level 3 of the launch table, learn_*_3.hip), measured against the EXPLORE kernels on
identical inputs, and a record of how the two targets learn.
   python tools/target_bench.py [--env mountaincar --env acrobot] [--agents 65536 --agents 4096] [--rounds 5] [--max-episodes 400]
                                [--quality-agents 4096] [--quality-episodes 60] [--out FILE]
cost     E agents of a demo, one start state each on the state grid (the workload of tools/explore_rows_bench.py), exploration rows
         set: 16 (epsilon, horizon) sets, epsilon 0.05 / 0.1 / 0.2 / 0.3 x horizon 2 / 4 / 8 / 16, agent e under set e mod 16.  Sides,
         alternating in one process, a fresh batch before each (outside the timed window), round 0 warms up, `rounds` timed rounds:
           x  frirl_hip_learn_train_explore                        the yardstick: its code is the parent's, unchanged
           s  frirl_hip_learn_train_target, an all-SARSA column    the TARGET kernels doing the same work, bit for bit
           q  frirl_hip_learn_train_target, an all-Q column        another trajectory: other steps, other rule counts
         Timed with device events around the call.  Per side: every round, the mean and the spread (max - min) of its own rounds.
quality  a constant epsilon = 0.1 population through the batch object (frirl_hip_batch_set_exploration, _set_target,
         frirl_hip_batch_train), then frirl_hip_batch_evaluate from every agent's own start: successes under either target after the
         same number of episodes.  A record, no claim: one seed, one run.
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
    sides = dict(x=None, s=frirl_amd.TargetRows(E, dev, target=np.zeros(E, dtype=np.uint8)), q=frirl_amd.TargetRows(E, dev, target=np.ones(E, dtype=np.uint8)))
    times = {k: [] for k in sides}
    last = {}
    for rnd in range(a.rounds + 1):                     # round 0 warms up every kernel variant the timed rounds launch
        for k, target in sides.items():
            prob, agent, envs = frirl_amd.fresh_batch(d, E, MAXR, dev, start_states=start, no_random=0, seed=SEED)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = frirl_amd.train_persistent(prob, agent, envs, max_episodes=a.max_episodes, budget=a.budget, explore=explore, target=target)
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
    out["s_over_x"] = out["s"]["mean"] / out["x"]["mean"]
    out["q_over_x"] = out["q"]["mean"] / out["x"]["mean"]
    out["s_minus_x_over_x_spread"] = (out["s"]["mean"] - out["x"]["mean"]) / max(out["x"]["spread"], 1e-12)
    out["s_equals_x_bit_for_bit"] = bool(torch.equal(last["s"]["rb"], last["x"]["rb"]) and torch.equal(last["s"]["steps"], last["x"]["steps"]))
    return out


def quality(env, E, a):
    lib = frirl_amd.lib()
    d = frirl_amd.demo_describe(env)
    rng = np.random.default_rng(3)
    start = np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))
    out = dict(mode="quality", env=env, agents=E, epsilon=0.1, episodes=a.quality_episodes)
    for name, tq in (("sarsa", frirl_amd.TARGET_SARSA), ("q", frirl_amd.TARGET_Q)):
        batch = frirl_amd.demo_batch_object(env, E, MAXR, start_states=start, seed=SEED)
        try:
            frirl_amd.batch_set_exploration(batch, epsilon=np.full(E, 0.1))
            frirl_amd.batch_set_target(batch, None, tq)
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
