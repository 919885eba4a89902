#!/usr/bin/env python3
"""The map-validated reduction over several candidate orders (frirl_hip_reduce_batch_map_orders) and the rule usage
(frirl_hip_rule_usage) against the one-order reduction (Problem.reduce_batch_map, strategy 1), on the 64 learned rule bases of
tools/reduce_bench.py (mountaincar and acrobot) at the points their greedy policies visit from 16 starts (frirl_hip_rollout_points,
only_successful = 1):
  * rules kept per order -- |Q| ascending, |Q| descending, least-used first, most-used first (the batch object's order set 15),
    reversed index and a fixed random permutation -- and by the best of the first four per agent
  * wall time per call: a warm-up and --reps timed repetitions, the sides alternating in one process, host clock around calls that end in
    a device synchronise, rule bases restored from a snapshot before every timed call (outside the window).  A window holds what a caller
    of the Problem method pays: the workspace's torch.empty and the ctypes marshalling besides the library call.  The orders are built
    outside the windows of the reductions; rule_usage and the four rule_order calls are timed on their own
python tools/reduce_orders_bench.py [--agents 64] [--starts 16] [--reps 3] [--spread 0.1] [--cap 512] [--only ENV]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import torch
import frirl_amd
import reduce_bench

NAMES = ["q_ascending", "q_descending", "least_used_first", "most_used_first", "reversed_index", "permutation"]


def leg(env, a, dev):
    E, K = a.agents, a.starts
    a.starts = [K]                                                    # reduce_bench.starts_inputs takes the list of its --starts
    d, prob, agent, envs, run, snap, restore, tens, ss, val, around = reduce_bench.starts_inputs(env, E, a, dev)
    a.starts = K
    ns = d["nstates"]
    starts = tens(val[:, :K, :].reshape(E * K, ns))
    points, count, overflow = prob.rollout_points(agent, K, cap=a.cap, only_successful=True, start_states=starts)[:3]
    torch.cuda.synchronize()
    active = (overflow == 0).to(torch.uint8)
    maxR = prob.maxR

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def build_orders():
        total, _, _ = prob.rule_usage(agent, points, point_count=count, active=active)
        return total, [prob.rule_order(None, False, active), prob.rule_order(None, True, active), prob.rule_order(total, False, active),
                       prob.rule_order(total, True, active)]

    (total, four), _ = timed(build_orders)
    nr = prob.nrules.cpu().numpy()
    extra = np.zeros((2, E, maxR), dtype=np.int32)
    for e in range(E):
        R = int(nr[e])
        extra[0, e, :R] = np.arange(R - 1, -1, -1)
        extra[1, e, :R] = np.random.default_rng(5).permutation(R)
    six = torch.stack(four + [tens(extra[0]), tens(extra[1])], dim=1).contiguous()
    four_t, one_t = six[:, :4].contiguous(), six[:, :1].contiguous()
    t = {k: [] for k in ("map", "orders_k1", "orders_k4", "usage", "usage_and_four_orders")}
    for rep in range(a.reps + 1):
        restore()
        (res_m, _), dt_m = timed(lambda: prob.reduce_batch_map(agent, points, point_count=count, active=active, strategy=1, rant=envs.rant))
        restore()
        (res_1, _, _), dt_1 = timed(lambda: prob.reduce_batch_map_orders(agent, points, one_t, point_count=count, active=active, rant=envs.rant))
        restore()
        (res_4, _, after_4), dt_4 = timed(lambda: prob.reduce_batch_map_orders(agent, points, four_t, point_count=count, active=active, rant=envs.rant))
        restore()
        _, dt_u = timed(lambda: prob.rule_usage(agent, points, point_count=count, active=active))
        _, dt_o = timed(build_orders)
        if rep:
            for k, v in zip(t, (dt_m, dt_1, dt_4, dt_u, dt_o)):
                t[k].append(round(v, 5))
    assert [(r.rules_after, r.tries) for r in res_m] == [(r.rules_after, r.tries) for r in res_1], "K = 1 with |Q| ascending is strategy 1"
    restore()
    res_6, _, after_6 = prob.reduce_batch_map_orders(agent, points, six, point_count=count, active=active, rant=envs.rant)
    restore()
    chosen = [r.chosen for r in res_4]
    print(json.dumps({
        "env": env, "agents": E, "starts": K, "cap": a.cap, "spread": a.spread, "converged": int((run.conv.converged == 1).sum()),
        "rules_before_sum": int(snap[1].sum()), "rules_max": int(snap[1].max()), "points_sum": int(count.sum()), "points_max": int(count.max()),
        "points_overflow_agents": int(overflow.sum()), "workgroups_k4": E * 4,
        "rules_after_sum_per_order": {n: int(after_6[:, k].sum()) for k, n in enumerate(NAMES)},
        "rules_after_sum_best_of_4": int(sum(r.rules_after for r in res_4)), "rules_after_sum_best_of_6": int(sum(r.rules_after for r in res_6)),
        "agents_won_by_order_of_4": {NAMES[k]: chosen.count(k) for k in range(4)}, "tries_sum_k1": int(sum(r.tries for r in res_1)),
        "map_s": t["map"], "orders_k1_s": t["orders_k1"], "orders_k4_s": t["orders_k4"], "usage_s": t["usage"],
        "usage_and_four_orders_s": t["usage_and_four_orders"],
        "k1_over_map_min": round(min(t["orders_k1"]) / min(t["map"]), 4), "k4_over_map_min": round(min(t["orders_k4"]) / min(t["map"]), 4),
        "k4_over_k1_min": round(min(t["orders_k4"]) / min(t["orders_k1"]), 4), "usage_over_map_min": round(min(t["usage"]) / min(t["map"]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for env in ([a.only] if a.only else ["mountaincar", "acrobot"]):
        leg(env, a, dev)


if __name__ == "__main__":
    main()
