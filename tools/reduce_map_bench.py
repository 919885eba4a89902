#!/usr/bin/env python3
"""The reduction validated on the policy map (frirl_hip_reduce_batch_map) against the reduction validated by replays from the same
start states (frirl_hip_reduce_batch_starts, n = 16, drop_bad_starts = 1), on the 64 learned rule bases of tools/reduce_bench.py
(mountaincar and acrobot, strategy 1):
  * every agent's 16 validation episodes are recorded (frirl_hip_rollout_record) and turned into its point list (frirl_hip_log_points,
    only_successful = 1: the counterpart of drop_bad_starts)
  * wall time per call: a warm-up and --reps timed repetitions, the two sides alternating in one process, host clock around calls that
    end in a device synchronise, rule bases restored from a snapshot before every timed call (outside the window).  The map side's
    window holds what a caller of Problem.reduce_batch_map pays: the workspace's torch.empty and the ctypes marshalling besides the
    library call.  Recording + point lists are timed on their own; map_over_starts_* compares the reductions alone (a caller who
    has the points), end_to_end_over_starts_min adds record + point lists to the map side (a caller who must record first)
  * rules kept, and how many of the independent test starts that the un-reduced rule bases solve are still solved afterwards
  * how many cells of the full state grid (frirl_amd.grid_points) change their greedy action under each reduction
  * how many of the validation episodes the map-reduced rule bases reproduce step for step (same steps and reward bits)
python tools/reduce_map_bench.py [--agents 64] [--starts 16] [--reps 3] [--spread 0.1] [--test-starts 32] [--cap 2048] [--only ENV]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import torch
import frirl_amd
import reduce_bench


def leg(env, a, dev):
    E, K = a.agents, a.starts
    a.starts = [K]                                                    # reduce_bench.starts_inputs takes the list of its --starts
    d, prob, agent, envs, run, snap, restore, tens, ss, val, around = reduce_bench.starts_inputs(env, E, a, dev)
    a.starts = K
    ns = d["nstates"]
    vk = tens(val[:, :K, :])
    test = tens(around(a.test_starts, 5).reshape(E * a.test_starts, ns))
    T = agent.desc.max_steps + 1

    def solved():
        _, reward, _, _ = prob.rollout_batch(agent, a.test_starts, start_states=test)
        torch.cuda.synchronize()
        return (reward > d["reward_good_above"]).cpu().numpy()

    def record():
        log = prob.rollout_record(agent, K, 1, T, start_states=vk.reshape(E * K, 1, ns))
        out = log.points(a.cap, only_successful=True)
        torch.cuda.synchronize()
        return log, out

    base = solved()
    grid = frirl_amd.grid_points(d, dev)                              # "how many cells of the full grid does a reduction change"
    cells = grid.expand(E, *grid.shape).contiguous()
    cells_before, _ = prob.policy_map(agent, cells, actconc=False)
    t_rec = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        log, (points, count, overflow) = record()
        if rep:
            t_rec.append(round(time.perf_counter() - t0, 4))
    steps0, reward0, ok0 = log.ep_steps.clone(), log.ep_reward.clone(), log.ep_success.clone()
    t_map, t_starts = [], []
    for rep in range(a.reps + 1):
        restore()
        t0 = time.perf_counter()
        res_m, kept_m = prob.reduce_batch_map(agent, points, point_count=count, strategy=1, rant=envs.rant)
        dt_m = time.perf_counter() - t0
        restore()
        t0 = time.perf_counter()
        _, res_s, per = prob.reduce_batch_starts(agent, 1, 0.0, a.depth, vk, drop_bad_starts=True, rant=envs.rant)
        dt_s = time.perf_counter() - t0
        if rep:
            t_map.append(round(dt_m, 4)); t_starts.append(round(dt_s, 4))
    lost_s = base & ~solved()                                         # the state after the last replay-validated run
    changed_s = int((prob.policy_map(agent, cells, actconc=False)[0] != cells_before).sum())
    restore()
    res_m, kept_m = prob.reduce_batch_map(agent, points, point_count=count, strategy=1, rant=envs.rant)
    lost_m = base & ~solved()
    changed_m = int((prob.policy_map(agent, cells, actconc=False)[0] != cells_before).sum())
    log1 = prob.rollout_record(agent, K, 1, T, start_states=vk.reshape(E * K, 1, ns))
    torch.cuda.synchronize()
    good = (ok0 == 1).view(-1)
    same = ((log1.ep_steps == steps0) & (log1.ep_reward == reward0) & (log1.ep_success == ok0)).view(-1)
    restore()
    print(json.dumps({
        "env": env, "agents": E, "starts": K, "strategy": 1, "spread": a.spread, "converged": int((run.conv.converged == 1).sum()),
        "rules_before_sum": int(snap[1].sum()), "record_and_points_s": t_rec, "points_sum": int(count.sum()), "points_max": int(count.max()),
        "points_overflow_agents": int(overflow.sum()), "records_sum": int(log.length.sum()), "validation_episodes_successful": int(good.sum()),
        "map_s": t_map, "starts_s": t_starts, "map_over_starts_min": round(min(t_map) / min(t_starts), 4),
        "map_over_starts_median": round(float(np.median(t_map) / np.median(t_starts)), 4),
        "end_to_end_over_starts_min": round((min(t_rec) + min(t_map)) / min(t_starts), 4),
        "map": {"rules_after_sum": int(sum(r.rules_after for r in res_m)), "tries_sum": int(sum(r.tries for r in res_m)),
                "test_lost": int(lost_m.sum()), "grid_cells_changed": changed_m, "validation_episodes_reproduced": int((same & good).sum())},
        "starts_n16": {"rules_after_sum": int(sum(r.rules_after for r in res_s)), "rounds_max": max(r.rounds for r in res_s),
                       "rollouts_sum": int(sum(r.rollouts for r in res_s)), "starts_used": int(sum(p.used for row in per for p in row)),
                       "depth": a.depth or frirl_amd.lib().frirl_hip_reduce_batch_starts_depth(E, d["A"], K), "test_lost": int(lost_s.sum()), "grid_cells_changed": changed_s},
        "grid_cells": int(cells.shape[0] * cells.shape[1]),
        "test_starts": int(base.size), "test_solved_before": int(base.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--test-starts", type=int, default=32)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for env in ([a.only] if a.only else ["mountaincar", "acrobot"]):
        leg(env, a, dev)


if __name__ == "__main__":
    main()
