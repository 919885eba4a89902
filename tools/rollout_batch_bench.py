#!/usr/bin/env python3
"""Population evaluation: n greedy roll-outs on EVERY agent's own rule base (frirl_hip_rollout_batch) against the stepped path.
The agents are trained by the persistent learner from diversified start states (as tools/learn2_bench.py); then, on the same rule
bases and rows:
   (a) stepped    frirl_hip_policy_batch_begin / _observe + frirl_hip_env_step: what the library offered before
   (b) tiled      frirl_hip_rollout_batch with rollout_batch_resident = 0
   (c) resident   frirl_hip_rollout_batch with rollout_batch_resident = 1
   (d) auto       frirl_hip_rollout_batch as shipped (rollout_batch_resident = -1)
   (e) lanes      acrobot, n = 1 only: frirl_hip_episode_run_lanes with evaluate = 1 (one episode per agent from its own start)
One JSON line per (env, E, n) with the call times (median of the repeats after a warm-up call, host clock around a synchronise),
env-steps/s and the counted FP64-issue fraction (rule visits from the returned steps, as the `evaluation` leg of bench.py).

   python tools/rollout_batch_bench.py                 every shape, each (env, E) in a child process under its own time limit
   python tools/rollout_batch_bench.py ENV E [n ...]   one (env, E) in this process
"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("acrobot", 4096), ("mountaincar", 4096), ("acrobot", 65536), ("mountaincar", 65536)]
LIMIT_S = 420          # per child

if len(sys.argv) < 3:
    for env, E in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), env, str(E), "1", "16"], timeout=LIMIT_S)
        if r.returncode != 0:          # a failed shape ends the run: nothing more is started on the device
            sys.exit(r.returncode)
    sys.exit(0)

import torch, frirl_amd

env, E = sys.argv[1], int(sys.argv[2])
ns_list = [int(a) for a in sys.argv[3:]] or [1, 16]
dev = torch.device("cuda", 0)
d = frirl_amd.demo_describe(env)
nant, A, nstates = d["nant"], d["A"], d["nstates"]
g = torch.Generator(device=dev).manual_seed(1)
start = torch.stack([torch.from_numpy(d["grids"][k]).to(dev)[torch.randint(0, len(d["grids"][k]), (E,), generator=g, device=dev)]
                     for k in range(nstates)], 1).contiguous()
prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 1024, dev, start_states=start)
torch.cuda.synchronize(); t0 = time.perf_counter()
frirl_amd.train_persistent(prob, agent, envs, max_episodes=400, budget=4096)
torch.cuda.synchronize(); train_s = time.perf_counter() - t0
R = prob.nrules.to(torch.float64)
lo = torch.tensor([d["grids"][k].min() for k in range(nstates)], dtype=torch.float64, device=dev)
hi = torch.tensor([d["grids"][k].max() for k in range(nstates)], dtype=torch.float64, device=dev)
PEAK_SLOTS = 3.93e13   # FP64 vector issue slots per second (78.6 TFLOP/s / 2), as tools/learn2_bench.py


def timed(fn, reps):
    fn(); torch.cuda.synchronize()                       # warm-up: code objects, allocator
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts), max(ts), out


def stepped(n, s):
    rows = frirl_amd.PolicyBatchRows(E, n, dev)
    states = s
    out = prob.policy_batch_begin(agent, rows, states)
    for t in range(agent.desc.max_steps):
        live = rows.done == 0
        obs, reward, success, _ = frirl_amd.env_step(agent, torch.where(live, out[0], torch.zeros_like(out[0])), states)
        prob.policy_batch_observe(agent, rows, obs, reward, success, out=out)
        states = torch.where(live[:, None], obs, states)
        if t % 16 == 15 and int((rows.done == 0).sum()) == 0:
            break
    return rows.ep_steps, rows.ep_reward, rows.success, states


for n in ns_list:
    Q = E * n
    s = start.repeat_interleave(n, 0)
    if n > 1:                                            # rows 1 .. n-1: the agent's start +- 0.15 * span, clipped; row 0 its own start
        off = (torch.rand((Q, nstates), dtype=torch.float64, device=dev, generator=g) * 2 - 1) * 0.15 * (hi - lo)
        off[::n] = 0
        s = (s + off).clamp(lo, hi)
    s = s.contiguous()
    rec = {"env": env, "agents": E, "rows_per_agent": n, "train_s": round(train_s, 3), "rules_mean": float(R.mean()), "rules_max": int(R.max()),
           "resident_capacity": frirl_amd.lib().frirl_hip_rollout_resident_rules(nant, A, 0, agent.desc.env_kind)}
    results = {}
    for name, opt in (("tiled", 0), ("resident", 1), ("auto", -1)):
        old = frirl_amd.set_option("rollout_batch_resident", opt)
        results[name] = timed(lambda: prob.rollout_batch(agent, n, start_states=s), 5)
        frirl_amd.set_option("rollout_batch_resident", old)
    results["stepped"] = timed(lambda: stepped(n, s), 1 if Q > 100000 else 3)
    steps = results["tiled"][3][0].to(torch.float64)
    for name in ("resident", "auto", "stepped"):
        o = results[name][3]
        same = bool((o[0] == results["tiled"][3][0]).all()) and bool((o[1] == results["tiled"][3][1]).all())
        rec[name + "_equals_tiled"] = same
    env_steps = float(steps.sum())
    visits = float(((steps + 1) * R.repeat_interleave(n)).sum())
    slots = visits * (14.4 * A + 2.0 * (nant - 1))
    rec.update(env_steps=env_steps, mean_steps=env_steps / Q, longest=int(steps.max()), successes=int((results["tiled"][3][2] == 1).sum()), rule_visits=visits)
    for name, (med, mn, mx, _) in results.items():
        rec[name] = {"ms": round(med * 1e3, 3), "min_ms": round(mn * 1e3, 3), "max_ms": round(mx * 1e3, 3), "env_steps_per_s": env_steps / med,
                     "fp64_issue_frac": slots / med / PEAK_SLOTS}
    if env == "acrobot" and n == 1:                      # the other baseline of the parent commit: one evaluate-mode episode per agent
        ev = frirl_amd.demo_agent(d, dev, evaluate=1)
        envs2 = frirl_amd.Envs(prob, dev, keep_rant=False, start_states=start)

        def lanes():
            frirl_amd.episode_begin(prob, ev, envs2)
            frirl_amd.episode_run_lanes(prob, ev, envs2, ev.desc.max_steps)
            return envs2.ep_steps
        med, mn, mx, lsteps = timed(lanes, 3)
        rec["lanes_evaluate"] = {"ms": round(med * 1e3, 3), "min_ms": round(mn * 1e3, 3), "max_ms": round(mx * 1e3, 3), "env_steps_per_s": float(lsteps.sum()) / med,
                                 "env_steps": float(lsteps.sum()), "steps_equal_tiled": float((lsteps == results["tiled"][3][0]).float().mean())}
    print(json.dumps(rec), flush=True)
