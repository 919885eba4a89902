#!/usr/bin/env python3
"""The point-keeping roll-out (frirl_hip_rollout_points) against the log path it replaces and against the plain roll-out, on rule bases
learned by the persistent learner (the 64 agents of tools/reduce_bench.py, mountaincar and acrobot; 16 starts per agent at +-10 % of
the span, only_successful = 1).  For E > 64 the 64 learned rule bases are REPEATED E / 64 times, every copy with start states of its
own: the learner is not what is measured here.
  (a) Problem.rollout_points into buffers of the caller (the wrapper's workspace torch.empty is inside the window)
  (b) frirl_hip_rollout_record + frirl_hip_log_points, every buffer (logs, point lists, workspace) allocated outside the window
  (c) Problem.rollout_batch, tiled form (rollout_batch_resident = 0), on the same rows: what keeping the points costs
  (d) at --big agents: (a) alone, with its workspace next to the bytes of records (b) would need
  (e) frirl_hip_batch_reduce_all_map against frirl_hip_batch_reduce_all_starts (drop_bad_starts = 1) on a batch object of 64 agents
      trained by frirl_hip_batch_train, its rule bases reloaded from a file before every timed call (outside the window)
One process; a warm-up and --reps timed repetitions, the sides alternating; host clock around calls that end in a device synchronise.
python tools/rollout_points_bench.py [--agents 64,4096] [--big 65536] [--starts 16] [--reps 3] [--spread 0.1] [--cap 512] [--only ENV]"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import torch
import frirl_amd
import reduce_bench


def row_sets(points, count):
    """per agent the sorted bytes of its rows"""
    p, c = points.cpu().numpy(), count.cpu().numpy()
    return [sorted(r.tobytes() for r in p[e, : c[e]]) for e in range(len(c))]


def timed(fn, reps):
    out, t = None, []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            t.append(round(time.perf_counter() - t0, 5))
    return out, t


def leg(env, a, dev):
    K, cap, L = a.starts, a.cap, frirl_amd.lib()
    a.starts = [K]
    d, prob64, agent, envs, run, snap, restore, tens, ss, val, around = reduce_bench.starts_inputs(env, 64, a, dev)
    a.starts = K
    ns, nant, T = d["nstates"], d["nant"], agent.desc.max_steps + 1
    lo = np.array([d["grids"][k].min() for k in range(ns)])
    hi = np.array([d["grids"][k].max() for k in range(ns)])
    own = ss.cpu().numpy()
    frirl_amd.set_option("rollout_batch_resident", 0)
    rec_bytes = 16 * ns + 17

    def problem(E):
        """the 64 rule bases E / 64 times, K starts per agent: row 0 the own start, the others own +- spread * span"""
        reps = E // 64
        rb = prob64.rb.repeat(reps, 1, 1).contiguous()
        nr = prob64.nrules.repeat(reps).contiguous()
        p = frirl_amd.Problem(prob64.u, prob64.ve, rb, nr)
        base = np.tile(own, (reps, 1))
        r = np.random.default_rng(17)
        x = np.clip(base[:, None, :] + r.uniform(-a.spread, a.spread, (E, K, ns)) * (hi - lo), lo, hi)
        x[:, 0, :] = base
        return p, tens(x.reshape(E * K, ns))

    def points_side(p, starts, E):
        out = (torch.zeros((E, cap, ns), dtype=torch.float64, device=dev), torch.empty((E,), dtype=torch.int32, device=dev),
               torch.empty((E,), dtype=torch.int32, device=dev))
        rows = (torch.empty((E * K,), dtype=torch.int32, device=dev), torch.empty((E * K,), dtype=torch.float64, device=dev),
                torch.empty((E * K,), dtype=torch.int32, device=dev))
        return lambda: p.rollout_points(agent, K, cap=cap, only_successful=True, start_states=starts, out=out, rows_out=rows)

    for E in a.agents:
        p, starts = problem(E)
        run_a = points_side(p, starts, E)
        log = frirl_amd.RolloutLog.empty(E * K, 1, T, ns, dev)
        pts_b = torch.zeros((E, cap, ns), dtype=torch.float64, device=dev)
        cnt_b, ovf_b = torch.empty((E,), dtype=torch.int32, device=dev), torch.empty((E,), dtype=torch.int32, device=dev)
        nb = L.frirl_hip_log_points_workspace_bytes(E, K, T)
        ws_b = torch.empty((nb,), dtype=torch.uint8, device=dev)
        lp = frirl_amd.LogPointsDesc(E, K, T, ns, cap, 1, log.obs.data_ptr(), log.q_obs.data_ptr(), log.success.data_ptr(), log.start.data_ptr(),
                                     log.length.data_ptr(), pts_b.data_ptr(), cnt_b.data_ptr(), ovf_b.data_ptr())
        st3 = starts.reshape(E * K, 1, ns)

        def run_b():
            p.rollout_record(agent, K, 1, T, start_states=st3, out=log)
            frirl_amd.check(L.frirl_hip_log_points(C.byref(lp), ws_b.data_ptr(), nb, None), "frirl_hip_log_points")

        out_c = (torch.empty((E * K,), dtype=torch.int32, device=dev), torch.empty((E * K,), dtype=torch.float64, device=dev),
                 torch.empty((E * K,), dtype=torch.int32, device=dev), torch.empty((E * K, ns), dtype=torch.float64, device=dev))
        run_c = lambda: p.rollout_batch(agent, K, start_states=starts, out=out_c)
        ta, tb, tc = [], [], []
        for rep in range(a.reps + 1):
            for fn, t in ((run_a, ta), (run_b, tb), (run_c, tc)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                if rep:
                    t.append(round(time.perf_counter() - t0, 5))
                if fn is run_a:
                    res_a = got
        pa, ca, oa, steps_a, reward_a, succ_a = res_a
        same = row_sets(pa, ca) == row_sets(pts_b, cnt_b) and int(oa.sum()) == 0 and int(ovf_b.sum()) == 0
        same_rows = bool((steps_a == out_c[0]).all() and (reward_a == out_c[1]).all() and (succ_a == out_c[2]).all())
        records = int(log.length.sum())
        list_bytes = int(ca.sum()) * ns * 8
        print(json.dumps({
            "leg": "points_vs_logs", "env": env, "agents": E, "starts": K, "cap": cap, "rules_sum": int(p.nrules.sum()),
            "points_s": ta, "record_and_log_points_s": tb, "rollout_batch_tiled_s": tc,
            "points_over_logs_min": round(min(ta) / min(tb), 4), "points_over_rollout_batch_min": round(min(ta) / min(tc), 4),
            "same_sets": bool(same), "rows_equal_rollout_batch": same_rows, "points_sum": int(ca.sum()), "points_max": int(ca.max()),
            "overflow_agents": int(oa.sum()), "records": records, "successful_rows": int((succ_a == 1).sum()),
            "bytes_written_points_side": {"lists": list_bytes + 8 * E, "rows": 16 * E * K, "segments_at_most": 2 * (list_bytes + 16 * E * ((K + 3) // 4)),
                                          "workspace_allocated": int(L.frirl_hip_rollout_points_workspace_bytes(nant, E, p.maxR, K, cap, d["A"]))},
            "bytes_written_logs_side": {"records": records * rec_bytes, "marks": records, "lists": list_bytes + 8 * E, "per_log": 20 * E * K,
                                        "log_buffers_allocated": E * K * T * rec_bytes}}), flush=True)
        del log, pts_b, ws_b, p, starts

    if a.big:
        E = a.big
        p, starts = problem(E)
        run_a = points_side(p, starts, E)
        res, t = timed(run_a, a.reps)
        ws = int(L.frirl_hip_rollout_points_workspace_bytes(nant, E, p.maxR, K, cap, d["A"]))
        print(json.dumps({"leg": "big", "env": env, "agents": E, "starts": K, "cap": cap, "points_s": t, "points_sum": int(res[1].sum()),
                          "points_max": int(res[1].max()), "overflow_agents": int(res[2].sum()), "workspace_bytes": ws,
                          "points_array_bytes": E * cap * ns * 8, "log_buffers_the_log_path_needs": E * K * T * rec_bytes,
                          "log_points_refuses": bool(E * K * T > 2 ** 31 - 1)}), flush=True)
        del p, starts, res

    # ---- (e) from the batch object --------------------------------------------------------------------------------------------------
    E = 64
    b = frirl_amd.demo_batch_object(env, E, 512, start_states=own)
    path = os.path.join(tempfile.mkdtemp(), "trained.bin")
    try:
        eps = C.c_int32()
        frirl_amd.check(L.frirl_hip_batch_train(b, 400, C.byref(eps)), "frirl_hip_batch_train")
        frirl_amd.check(L.frirl_hip_batch_save_rulebases(b, path.encode()), "save")
        x = np.ascontiguousarray(np.clip(own[:, None, :] + np.random.default_rng(17).uniform(-a.spread, a.spread, (E, K, ns)) * (hi - lo), lo, hi))
        x[:, 0, :] = own
        DP = C.POINTER(C.c_double)
        rm, tot = (frirl_amd.ReduceMapResult * E)(), frirl_amd.ReduceMapTotals()
        rs, per, nred = (frirl_amd.ReduceResult * E)(), (frirl_amd.ReduceStartResult * (E * K))(), C.c_int32()
        tm, ts = [], []
        for rep in range(a.reps + 1):
            for side, t in (("map", tm), ("starts", ts)):
                nrec = C.c_int32()
                frirl_amd.check(L.frirl_hip_batch_load_rulebases(b, path.encode(), C.byref(nrec)), "load")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if side == "map":
                    frirl_amd.check(L.frirl_hip_batch_reduce_all_map(b, 1, K, x.ctypes.data_as(DP), 1, cap, rm, C.byref(tot)), "reduce_all_map")
                else:
                    frirl_amd.check(L.frirl_hip_batch_reduce_all_starts(b, 1, 0.0, 0, K, x.ctypes.data_as(DP), 1, rs, per, C.byref(nred)), "reduce_all_starts")
                if rep:
                    t.append(round(time.perf_counter() - t0, 5))
        print(json.dumps({"leg": "batch_object", "env": env, "agents": E, "starts": K, "episodes_trained": eps.value, "reduce_all_map_s": tm,
                          "reduce_all_starts_s": ts, "map_over_starts_min": round(min(tm) / min(ts), 4),
                          "map": {"agents_reduced": tot.agents_reduced, "agents_overflow": tot.agents_overflow, "agents_without_points": tot.agents_without_points,
                                  "rules_before": tot.rules_before, "rules_after": tot.rules_after, "points": tot.points},
                          "starts": {"agents_reduced": nred.value, "rules_before": sum(r.rules_before for r in rs), "rules_after": sum(r.rules_after for r in rs),
                                     "starts_used": sum(q.used for q in per), "replays": sum(r.rollouts for r in rs)}}), flush=True)
    finally:
        L.frirl_hip_batch_destroy(b)
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(os.path.dirname(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default="64,4096")
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--test-starts", type=int, default=32)
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    a.agents = [int(x) for x in a.agents.split(",") if x]
    assert all(E % 64 == 0 for E in a.agents + [a.big]), "agent counts are multiples of the 64 learned rule bases"
    dev = torch.device("cuda:0")
    for env in ([a.only] if a.only else ["mountaincar", "acrobot"]):
        leg(env, a, dev)


if __name__ == "__main__":
    main()
