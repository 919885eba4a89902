#!/usr/bin/env python3
"""Recorded roll-outs (frirl_hip_rollout_record) against what the library offered before, and the effect of teaching from the best agent.

record ENV E   E agents trained by the persistent learner from diversified start states; then ONE greedy episode per agent (E logs, n = 1,
               K = 1, T = max_steps + 1) from its own start state, three ways on the same rule bases and rows:
   (a) record    frirl_hip_rollout_record
   (b) stepped   frirl_hip_policy_batch_begin / _observe + frirl_hip_env_step + the copies of every step into the same log arrays
   (c) rollout   frirl_hip_rollout_batch with rollout_batch_resident = 0: the same episodes without the records
               (b) and (c) are code of the parent commit.  One JSON line: call times (median, min, max of the repeats after a warm-up call,
               host clock around a synchronise), env-steps/s, and whether the three agree.
teach E EPISODES   two library-owned batches of E diversified mountain-car agents, each trained EPISODES / 2 + EPISODES / 2 episodes;
               the second gets one frirl_hip_batch_teach round in between (teacher = frirl_hip_batch_evaluate's best agent, 8 episodes).
               One JSON line: converged agents, episodes and rules of both batches.

   python tools/rollout_record_bench.py                  every shape, each in a child process under its own time limit
"""
import ctypes as C
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS = [["record", "acrobot", "64"], ["record", "acrobot", "4096"], ["record", "cartpole", "64"], ["teach", "4096", "300"], ["record", "cartpole", "4096"]]
LIMIT_S = 300          # per child
TRAIN_EPISODES = {"acrobot": 200, "cartpole": 40, "mountaincar": 200}      # enough for rule bases of a realistic size; not to convergence

if len(sys.argv) < 2:
    for job in JOBS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + job, timeout=LIMIT_S)
        if r.returncode != 0:          # a failed shape ends the run: nothing more is started on the device
            sys.exit(r.returncode)
    sys.exit(0)

import numpy as np
import torch, frirl_amd

dev = torch.device("cuda", 0)


def diversified(d, E, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.stack([torch.from_numpy(d["grids"][k]).to(dev)[torch.randint(0, len(d["grids"][k]), (E,), generator=g, device=dev)]
                        for k in range(d["nstates"])], 1).contiguous()


def timed(fn, reps):
    fn(); torch.cuda.synchronize()                       # warm-up: code objects, allocator
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts), max(ts), out


def record_job(env, E):
    d = frirl_amd.demo_describe(env)
    ns = d["nstates"]
    start = diversified(d, E)
    prob, agent, envs = frirl_amd.demo_fresh_batch(env, E, 2048 if env == "cartpole" else 1024, dev, start_states=start)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    frirl_amd.train_persistent(prob, agent, envs, max_episodes=TRAIN_EPISODES[env], budget=4096)
    torch.cuda.synchronize(); train_s = time.perf_counter() - t0
    R = prob.nrules.to(torch.float64)
    T = agent.desc.max_steps + 1
    log_a = frirl_amd.RolloutLog.empty(E, 1, T, ns, dev)
    log_b = frirl_amd.RolloutLog.empty(E, 1, T, ns, dev)
    starts3 = start.reshape(E, 1, ns).contiguous()

    def record():
        return prob.rollout_record(agent, 1, 1, T, start_states=starts3, out=log_a)

    def put(lg, t, live, obs, q, action_idx, reward, success, first):
        lg.obs[:, t] = torch.where(live[:, None], obs, lg.obs[:, t])
        lg.q_obs[:, t] = torch.where(live[:, None], q, lg.q_obs[:, t])
        lg.action[:, t] = torch.where(live, action_idx, lg.action[:, t])
        lg.reward[:, t] = torch.where(live, reward, lg.reward[:, t])
        lg.success[:, t] = torch.where(live, success, lg.success[:, t])
        lg.start[:, t] = torch.where(live, torch.full_like(lg.start[:, t], first), lg.start[:, t])

    def stepped():
        rows = frirl_amd.PolicyBatchRows(E, 1, dev)
        states = start
        out = prob.policy_batch_begin(agent, rows, states)
        live = rows.done == 0
        zero, zi = torch.zeros_like(states), torch.zeros((E,), dtype=torch.int32, device=dev)
        put(log_b, 0, live, states, zero, out[1], torch.zeros((E,), dtype=torch.float64, device=dev), zi, 1)
        for t in range(agent.desc.max_steps):
            live = rows.done == 0
            obs, reward, success, q = frirl_amd.env_step(agent, torch.where(live, out[0], torch.zeros_like(out[0])), states)
            prob.policy_batch_observe(agent, rows, obs, reward, success, q_obs=q if env == "cartpole" else None, out=out)
            put(log_b, t + 1, live, obs, q, out[1], reward, success, 0)
            states = torch.where(live[:, None], obs, states)
            if t % 16 == 15 and int((rows.done == 0).sum()) == 0:
                break
        log_b.length.copy_(rows.ep_steps + 1)
        log_b.ep_steps[:, 0] = rows.ep_steps
        log_b.ep_reward[:, 0] = rows.ep_reward
        log_b.ep_success[:, 0] = rows.success
        return log_b

    def rollout():
        old = frirl_amd.set_option("rollout_batch_resident", 0)
        try:
            return prob.rollout_batch(agent, 1, start_states=start)
        finally:
            frirl_amd.set_option("rollout_batch_resident", old)

    # (a) and (c) differ by little: their repeats alternate, so that a drift of the shared machine hits both alike
    record(); rollout(); torch.cuda.synchronize()
    ts = {"record": [], "rollout": []}
    for _ in range(7):
        for name, fn in (("record", record), ("rollout", rollout)):
            torch.cuda.synchronize(); t = time.perf_counter()
            last = fn()
            torch.cuda.synchronize(); ts[name].append(time.perf_counter() - t)
            ts[name + "_out"] = last
    results = {name: (statistics.median(ts[name]), min(ts[name]), max(ts[name]), ts[name + "_out"]) for name in ("record", "rollout")}
    results["stepped"] = timed(stepped, 1 if E > 1000 else 3)
    a, b, c = results["record"][3], results["stepped"][3], results["rollout"][3]
    steps = a.ep_steps[:, 0]
    valid = torch.arange(T, device=dev)[None, :] < a.length[:, None]
    same_b = bool((a.length == b.length).all()) and bool((a.ep_reward == b.ep_reward).all())
    for name in ("obs", "q_obs", "action", "reward", "success", "start"):
        x, y = getattr(a, name), getattr(b, name)
        m = valid if x.dim() == 2 else valid[:, :, None]
        same_b = same_b and bool(((x == y) | ~m).all())
    same_c = bool((steps == c[0]).all()) and bool((a.ep_reward[:, 0] == c[1]).all()) and bool((a.ep_success[:, 0] == c[2]).all())
    env_steps = float(steps.sum())
    rec = {"job": "record", "env": env, "logs": E, "train_s": round(train_s, 3), "rules_mean": float(R.mean()), "rules_max": int(R.max()),
           "env_steps": env_steps, "mean_steps": env_steps / E, "longest": int(steps.max()), "successes": int((a.ep_success == 1).sum()),
           "log_bytes": int(a.length.sum()) * (2 * ns * 8 + 8 + 4 + 4 + 1), "stepped_equals_record": same_b, "rollout_equals_record": same_c}
    for name, (med, mn, mx, _) in results.items():
        rec[name] = {"ms": round(med * 1e3, 3), "min_ms": round(mn * 1e3, 3), "max_ms": round(mx * 1e3, 3), "env_steps_per_s": env_steps / med}
    rec["record_over_rollout"] = results["record"][0] / results["rollout"][0]
    rec["stepped_over_record"] = results["stepped"][0] / results["record"][0]
    print(json.dumps(rec), flush=True)


def teach_job(E, episodes):
    L = frirl_amd.lib()
    env, K, M = "mountaincar", 1, 8                                   # K = 1: every agent is scored on the start state it trains from
    d = frirl_amd.demo_describe(env)
    start = diversified(d, E).cpu().numpy()
    half = episodes // 2
    out = {"job": "teach", "env": env, "agents": E, "episodes_per_half": half, "teach_episodes": M}
    for name in ("plain", "taught"):
        b = frirl_amd.demo_batch_object(env, E, 1024, start_states=start)
        try:
            t0 = time.perf_counter()
            ran = C.c_int32()
            st = frirl_amd.BatchStats()
            frirl_amd.check(L.frirl_hip_batch_train(b, half + 1, C.byref(ran)), "frirl_hip_batch_train")
            frirl_amd.check(L.frirl_hip_batch_stats(b, C.byref(st)), "frirl_hip_batch_stats")
            rec = {"converged_half": int(st.converged), "rules_mean_half": st.rules_sum / E}
            if name == "taught":
                best = C.c_int32()
                sc = (frirl_amd.RolloutScore * E)()
                frirl_amd.check(L.frirl_hip_batch_evaluate(b, K, None, sc, C.byref(best)), "frirl_hip_batch_evaluate")
                t1 = time.perf_counter()
                res = frirl_amd.batch_teach(b, best.value, M, passes=1)
                rec.update(teacher=best.value, teacher_successes=int(sc[best.value].successes), teach_s=round(time.perf_counter() - t1, 4),
                           **{f: int(getattr(res, f)) for f, _ in frirl_amd.TeachResult._fields_ if f != "teacher"})
                frirl_amd.check(L.frirl_hip_batch_stats(b, C.byref(st)), "frirl_hip_batch_stats")
                rec["converged_after_teach"] = int(st.converged)
            frirl_amd.check(L.frirl_hip_batch_train(b, episodes - half + 1, C.byref(ran)), "frirl_hip_batch_train")
            frirl_amd.check(L.frirl_hip_batch_stats(b, C.byref(st)), "frirl_hip_batch_stats")
            sc = (frirl_amd.RolloutScore * E)()
            frirl_amd.check(L.frirl_hip_batch_evaluate(b, K, None, sc, None), "frirl_hip_batch_evaluate")
            rec.update(converged=int(st.converged), episodes_max=int(st.episodes_max), rules_mean=st.rules_sum / E, full_agents=int(st.full_agents),
                       env_steps=int(st.total_env_steps), agents_succeeding_greedily=sum(1 for s in sc if s.successes == s.rows and s.rows > 0),
                       wall_s=round(time.perf_counter() - t0, 3))
            out[name] = rec
        finally:
            L.frirl_hip_batch_destroy(b)
    print(json.dumps(out), flush=True)


if sys.argv[1] == "record":
    record_job(sys.argv[2], int(sys.argv[3]))
elif sys.argv[1] == "teach":
    teach_job(int(sys.argv[2]), int(sys.argv[3]))
else:
    sys.exit("usage: rollout_record_bench.py [record ENV E | teach E EPISODES]")
