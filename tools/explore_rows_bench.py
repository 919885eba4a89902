#!/usr/bin/env python3
"""What the exploration columns cost the users of the ROWS learner kernels, and what an exploration sweep in one run saves: E agents
of a demo, one start state each on the state grid (the workload of tools/hparam_rows_bench.py), through the persistent learner.
   python tools/explore_rows_bench.py cost  [env] [E] [budget] [max_episodes] [reps]
   python tools/explore_rows_bench.py sweep [env] [E] [budget] [max_episodes] [reps]
cost   sides alternating in one process, a fresh batch before each (outside the timed window), one warm-up round and `reps` timed:
         a  frirl_hip_learn_train
         b  frirl_hip_learn_train_rows, every column equal to the agent's own values (side b of tools/hparam_rows_bench.py)
         x  frirl_hip_learn_train_explore, an epsilon column of zeros and no hyper-parameter rows (where the binding has it)
       This mode uses nothing newer than rows=, so the same file runs against a checkout of the parent commit (put that checkout
       first on PYTHONPATH): b here against b there is what the two NULL tests per step cost the rows users.
sweep  c  16 (epsilon, horizon) sets, epsilon 0.05 / 0.1 / 0.2 / 0.3 x horizon 2 / 4 / 8 / 16, agent e under set e mod 16, one run
       d  what the sweep cost before: 16 runs of E / 16 agents (the agents and start states of that set in c), each with the set's
          epsilon as the batch's and its horizon as horizon_all, summed.  Compared by counts, not bits (other lane-group sizes).
Times are host clocks around runs that end in a device synchronise.  One JSON line per side and one per set of the sweep."""
import json, os, sys, time
if not os.environ.get("FRIRL_BENCH_NO_PATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch, frirl_amd

mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
env = sys.argv[2] if len(sys.argv) > 2 else "acrobot"
E = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
budget = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
max_episodes = int(sys.argv[5]) if len(sys.argv) > 5 else 400
reps = int(sys.argv[6]) if len(sys.argv) > 6 else 3
NSETS, MAXR, SEED = 16, 1024, 1265
assert mode in ("cost", "sweep") and E % NSETS == 0
dev = torch.device("cuda", 0)
d = frirl_amd.demo_describe(env)
g = torch.Generator(device=dev).manual_seed(1)
start = torch.stack([torch.from_numpy(d["grids"][k]).to(dev)[torch.randint(0, len(d["grids"][k]), (E,), generator=g, device=dev)]
                     for k in range(d["nstates"])], 1).contiguous()


def run(starts, agent_kw=None, **train_kw):
    """One timed construct run on a fresh batch: (seconds, result tensors)."""
    prob, agent, envs = frirl_amd.fresh_batch(d, starts.shape[0], MAXR, dev, start_states=starts, **(agent_kw or {}))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = frirl_amd.train_persistent(prob, agent, envs, max_episodes=max_episodes, budget=budget, **train_kw)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return dt, dict(nrules=prob.nrules, steps=r.steps_total, episodes=r.conv.episodes, converged=r.conv.converged, reward=r.conv.prev_reward, launches=r.launches)


if mode == "cost":
    own = {k: np.full(E, d[k]) for k in ("alpha", "gamma", "qdiff_pos", "qdiff_neg", "weight_thr")}
    rows_own = frirl_amd.HparamRows(E, dev, alpha=own["alpha"], gamma=own["gamma"], qdiff_pos_boundary=own["qdiff_pos"], qdiff_neg_boundary=own["qdiff_neg"],
                                    weight_significant=own["weight_thr"], skip_rules=np.full(E, d["skip_rules"], dtype=np.int32))
    explore0 = frirl_amd.ExploreRows(E, dev, epsilon=np.zeros(E)) if hasattr(frirl_amd, "ExploreRows") else None
    times = dict(a=[], b=[], x=[])
    for rep in range(reps + 1):                 # round 0 warms up every kernel variant the timed rounds launch
        ta, ra = run(start)
        tb, rb_ = run(start, rows=rows_own)
        tx = run(start, explore=explore0)[0] if explore0 is not None else None
        if rep:
            times["a"].append(ta); times["b"].append(tb)
            if tx is not None:
                times["x"].append(tx)
    print(json.dumps(dict(mode=mode, env=env, agents=E, budget=budget, max_episodes=max_episodes, package=os.path.dirname(frirl_amd.__file__), a_s=times["a"], b_s=times["b"],
                          x_s=times["x"], b_over_a=[b / a for a, b in zip(times["a"], times["b"])], env_steps=int(ra["steps"].sum()), launches=ra["launches"],
                          b_steps_equal_a=bool(torch.equal(ra["steps"], rb_["steps"])))))
else:
    sets = [(eps, h) for eps in (0.05, 0.1, 0.2, 0.3) for h in (2, 4, 8, 16)]
    kw = dict(no_random=0, seed=SEED)
    mixed = frirl_amd.ExploreRows(E, dev, epsilon=np.array([sets[e % NSETS][0] for e in range(E)]), horizon=np.array([sets[e % NSETS][1] for e in range(E)], dtype=np.int32))
    tcs, tds = [], []
    for rep in range(reps + 1):
        tc, rc = run(start, agent_kw=kw, explore=mixed)
        td, d_converged, d_steps = 0.0, [], []
        for s, (eps, h) in enumerate(sets):
            idx = torch.arange(s, E, NSETS, device=dev)
            t, rd = run(start[idx].contiguous(), agent_kw=dict(kw, epsilon=eps), explore=frirl_amd.ExploreRows(E // NSETS, dev, horizon_all=h))
            td += t
            d_converged.append(int(rd["converged"].sum())); d_steps.append(int(rd["steps"].sum()))
        if rep:
            tcs.append(tc); tds.append(td)
    print(json.dumps(dict(mode=mode, env=env, agents=E, budget=budget, max_episodes=max_episodes, c_s=tcs, d_s_summed=tds, d_over_c=[x / c for c, x in zip(tcs, tds)],
                          c_env_steps=int(rc["steps"].sum()), d_env_steps=sum(d_steps), c_converged=int(rc["converged"].sum()), d_converged=sum(d_converged), c_launches=rc["launches"])))
    for s, (eps, h) in enumerate(sets):
        idx = torch.arange(s, E, NSETS, device=dev)
        print(json.dumps(dict(set=s, epsilon=eps, horizon=h, agents=int(idx.numel()), converged=int(rc["converged"][idx].sum()), converged_d=d_converged[s],
                              mean_episodes=float(rc["episodes"][idx].float().mean()), mean_rules=float(rc["nrules"][idx].float().mean()),
                              mean_last_reward=float(rc["reward"][idx].mean()), env_steps=int(rc["steps"][idx].sum()))))
