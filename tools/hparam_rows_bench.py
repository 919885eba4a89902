#!/usr/bin/env python3
"""What per-agent hyper-parameter rows cost, and what a sweep in one run saves: E agents of a demo, one start state each on the state
grid (the diversified run of tools/learn2_bench.py), through the persistent learner.
   python tools/hparam_rows_bench.py [env] [E] [budget] [max_episodes] [reps]
Sides, alternating in one process, a fresh batch before each (outside the timed window), one warm-up round and `reps` timed ones:
  a, a2  frirl_hip_learn_train, twice: a2 / a is the spread of a round, and "a2 equals a bit for bit" says whether the run itself
         repeats (the queue orders agents of equal rule count by atomics, so at sizes where a launch cannot take every live agent
         two runs may cut an agent's run at different places and give it other lane-group sizes: last bits of the sums, see learn.hip)
  b      frirl_hip_learn_train_rows, every column equal to the agent's own values: equals (a) bit for bit where a2 does;
         b / a = the feature's cost
  c      a sweep: 16 sets, alpha x weight_significant around the demo's values, agent e under set e mod 16
  d      what the sweep cost before: 16 runs of (a) with E / 16 agents each (the agents and start states of that set in c), summed.
         A run of E / 16 agents gives its agents other lane-group sizes than the mixed run, so the comparison with (c) is by
         converged agents and environment steps per set, not by bits
Times are host clocks around runs that end in a device synchronise.  One JSON line per side and one per set of the sweep."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch, frirl_amd

env = sys.argv[1] if len(sys.argv) > 1 else "acrobot"
E = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
budget = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
max_episodes = int(sys.argv[4]) if len(sys.argv) > 4 else 400
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
NSETS, MAXR = 16, 1024
assert E % NSETS == 0
dev = torch.device("cuda", 0)
d = frirl_amd.demo_describe(env)
g = torch.Generator(device=dev).manual_seed(1)
start = torch.stack([torch.from_numpy(d["grids"][k]).to(dev)[torch.randint(0, len(d["grids"][k]), (E,), generator=g, device=dev)]
                     for k in range(d["nstates"])], 1).contiguous()
sets = [dict(alpha=d["alpha"] * fa, weight_thr=w) for fa in (0.5, 0.7, 0.85, 1.0) for w in (0.02, 0.035, 0.05, 0.08)]
own = {k: np.full(E, d[k]) for k in ("alpha", "gamma", "qdiff_pos", "qdiff_neg", "weight_thr")}
rows_own = frirl_amd.HparamRows(E, dev, alpha=own["alpha"], gamma=own["gamma"], qdiff_pos_boundary=own["qdiff_pos"], qdiff_neg_boundary=own["qdiff_neg"],
                                weight_significant=own["weight_thr"], skip_rules=np.full(E, d["skip_rules"], dtype=np.int32))
rows_sweep = frirl_amd.HparamRows(E, dev, alpha=np.array([sets[e % NSETS]["alpha"] for e in range(E)]),
                                  weight_significant=np.array([sets[e % NSETS]["weight_thr"] for e in range(E)]))


def run(desc, starts, rows):
    """One timed construct run on a fresh batch: (seconds, result tensors)."""
    prob, agent, envs = frirl_amd.fresh_batch(desc, starts.shape[0], MAXR, dev, start_states=starts)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = frirl_amd.train_persistent(prob, agent, envs, max_episodes=max_episodes, budget=budget, rows=rows)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return dt, dict(rb=prob.rb, nrules=prob.nrules, steps=r.steps_total, episodes=r.conv.episodes, converged=r.conv.converged, reward=r.conv.prev_reward,
                    launches=r.launches)


def same(x, y):
    return all(torch.equal(x[k].view(torch.int64) if x[k].dtype == torch.float64 else x[k], y[k].view(torch.int64) if y[k].dtype == torch.float64 else y[k])
               for k in ("rb", "nrules", "steps", "episodes", "converged", "reward"))


times = dict(a=[], a2=[], b=[], c=[], d=[])
equal_aa, equal_ab = [], []
for rep in range(reps + 1):                 # round 0 warms up every kernel variant the timed rounds launch
    ta, ra = run(d, start, None)
    tb, rb_ = run(d, start, rows_own)
    ta2, ra2 = run(d, start, None)
    tc, rc = run(d, start, rows_sweep)
    equal_ab.append(same(ra, rb_))
    equal_aa.append(same(ra, ra2))
    del rb_, ra2
    td, d_converged, d_steps = 0.0, [], []
    for s in range(NSETS):
        idx = torch.arange(s, E, NSETS, device=dev)
        t, rd = run(dict(d, **sets[s]), start[idx].contiguous(), None)
        td += t
        d_converged.append(int(rd["converged"].sum()))
        d_steps.append(int(rd["steps"].sum()))
        del rd
    if rep:
        for k, t in zip(("a", "a2", "b", "c", "d"), (ta, ta2, tb, tc, td)):
            times[k].append(t)
for k, r in (("a", ra), ("c", rc)):
    print(json.dumps(dict(side=k, env=env, agents=E, budget=budget, max_episodes=max_episodes, wall_s=times[k], env_steps=int(r["steps"].sum()),
                          launches=r["launches"], converged=int(r["converged"].sum()))))
print(json.dumps(dict(side="a2", env=env, wall_s=times["a2"], equals_a_bit_for_bit=equal_aa, ratio_a2_over_a=[x / a for a, x in zip(times["a"], times["a2"])])))
print(json.dumps(dict(side="b", env=env, wall_s=times["b"], equals_a_bit_for_bit=equal_ab, ratio_b_over_a=[b / a for a, b in zip(times["a"], times["b"])])))
print(json.dumps(dict(side="d", env=env, runs=NSETS, agents_per_run=E // NSETS, wall_s_summed=times["d"], converged_per_set=d_converged, env_steps_per_set=d_steps,
                      ratio_d_over_c=[x / c for c, x in zip(times["c"], times["d"])])))
for s in range(NSETS):
    idx = torch.arange(s, E, NSETS, device=dev)
    print(json.dumps(dict(set=s, alpha=sets[s]["alpha"], weight_significant=sets[s]["weight_thr"], agents=int(idx.numel()), converged=int(rc["converged"][idx].sum()),
                          mean_episodes=float(rc["episodes"][idx].float().mean()), max_episodes=int(rc["episodes"][idx].max()),
                          mean_rules=float(rc["nrules"][idx].float().mean()), mean_last_reward=float(rc["reward"][idx].mean()), env_steps=int(rc["steps"][idx].sum()))))
