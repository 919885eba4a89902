#!/usr/bin/env python3
"""The selection leg of one generation, on the device against through the host, on the same population:
  (a) frirl_hip_select_plan_device alone (device events) against the host leg it replaces: the scores copied to the host,
      frirl_hip_select_plan, the src table copied back (host clock around the synchronised copies)
  (b) the whole leg: frirl_hip_batch_evolve_step(spec = NULL) against frirl_hip_batch_select (host clock; both synchronise inside)
python tools/evolve_bench.py [--env mountaincar --env acrobot] [--agents 4096 --agents 65536] [--rounds 5] [--out profiles/r31_evolve.md]
The population is the recipe of tools/select_bench.py as a library-owned batch: 64 start states spread over the state grids, agent e
starts at state perm[e] mod 64 and trains --episodes greedy episodes, so the batch holds the 64 trained rule bases tiled and shuffled.
Half of the agents are replaced by the other half (parents = replace = E / 2), n = 1 evaluation row per agent at its own start state.
(b) runs on twin batches: a selection changes the batch, and with spec = NULL both calls leave the same bytes (tests/test_hip_evolve.py),
so in every round both sides start from the same state.  Round 0 warms up; within a round the sides alternate, the order flipping
every round.  Reported: every round, the minimum, spread = (max - min) / min.  (a) also checks that both forms give the same src."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
import frirl_amd


def trained_batch(env, E, a, d):
    rng = np.random.default_rng(11)
    E0 = min(64, E)
    start0 = np.stack([rng.choice(d["grids"][k], E0) for k in range(d["nstates"])], 1)
    start = np.ascontiguousarray(start0[(np.arange(E) % E0)[rng.permutation(E)]])
    b = frirl_amd.demo_batch_object(env, E, a.max_rules, start_states=start)
    ran = C.c_int32(0)
    frirl_amd.check(frirl_amd.lib().frirl_hip_batch_train(b, a.episodes + 1, C.byref(ran)), "frirl_hip_batch_train")
    return b, start


def stats(ts):
    best = min(ts)
    return {"us": [round(t * 1e6, 1) for t in ts], "min_us": round(best * 1e6, 1), "spread": round((max(ts) - best) / best, 3)}


def verdict(dev, host):
    """no slower than the host side by more than the larger of the two measured spreads"""
    margin = max(dev["spread"] * dev["min_us"], host["spread"] * host["min_us"])
    return {"host_over_device": round(host["min_us"] / dev["min_us"], 2), "margin_us": round(margin, 1), "holds": bool(dev["min_us"] <= host["min_us"] + margin)}


def bench(env, E, a, dev):
    L = frirl_amd.lib()
    d = frirl_amd.demo_describe(env)
    parents = replace = E // 2
    one, start = trained_batch(env, E, a, d)
    two, _ = trained_batch(env, E, a, d)
    starts = np.ascontiguousarray(start[:, None, :])
    DP, I32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    try:
        # ---- (a) the plan alone, on the scores of this population ----------------------------------------------------------------
        host_scores = (frirl_amd.RolloutScore * E)()
        frirl_amd.check(L.frirl_hip_batch_evaluate(one, 1, starts.ctypes.data_as(DP), host_scores, None), "frirl_hip_batch_evaluate")
        scores = torch.from_numpy(np.frombuffer(bytes(host_scores), dtype=np.uint8).reshape(E, C.sizeof(frirl_amd.RolloutScore)).copy()).to(dev)
        src_d = torch.empty(E, dtype=torch.int32, device=dev)
        rank_d, info_d = torch.empty_like(src_d), torch.empty(4, dtype=torch.int32, device=dev)
        stream = frirl_amd._stream(None)
        t_dev, t_host = [], []

        def plan_device():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            frirl_amd.check(L.frirl_hip_select_plan_device(scores.data_ptr(), E, None, parents, replace, src_d.data_ptr(), rank_d.data_ptr(), info_d.data_ptr(), stream),
                            "frirl_hip_select_plan_device")
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e-3

        def plan_host():
            src_h = np.empty(E, dtype=np.int32)
            t0 = time.perf_counter()
            sc = scores.cpu().numpy()                                                   # synchronised D2H of E * 40 bytes
            frirl_amd.check(L.frirl_hip_select_plan(sc.ctypes.data_as(C.POINTER(frirl_amd.RolloutScore)), E, None, parents, replace, src_h.ctypes.data_as(I32), None),
                            "frirl_hip_select_plan")
            up = torch.from_numpy(src_h).to(dev)                                        # H2D of E * 4 bytes
            torch.cuda.synchronize()
            return time.perf_counter() - t0, up

        for rnd in range(a.rounds + 1):
            for side in (("d", "h") if rnd % 2 == 0 else ("h", "d")):
                torch.cuda.synchronize()
                if side == "d":
                    t = plan_device()
                    if rnd:
                        t_dev.append(t)
                else:
                    t, up = plan_host()
                    if rnd:
                        t_host.append(t)
        same = bool(torch.equal(up, src_d)) and info_d.tolist()[:2] == [E, 0]
        successes = np.array([s.successes for s in host_scores])
        out = {"env": env, "agents": E, "parents": parents, "replace": replace, "pair_tests": E * E, "agents_successful": int((successes > 0).sum()),
               "plan_same_src": same, "plan_device": stats(t_dev), "plan_host_leg": stats(t_host)}
        out["plan_verdict"] = verdict(out["plan_device"], out["plan_host_leg"])
        out["plan_device"]["pair_tests_per_s"] = round(E * E / min(t_dev) / 1e9, 1)     # G pair tests / s

        # ---- (b) the whole selection leg on twin batches --------------------------------------------------------------------------------
        t_step, t_select = [], []
        res_e, res_s = frirl_amd.EvolveResult(), frirl_amd.SelectResult()
        agree = True
        for rnd in range(a.rounds + 1):
            for side in (("e", "s") if rnd % 2 == 0 else ("s", "e")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if side == "e":
                    frirl_amd.check(L.frirl_hip_batch_evolve_step(one, 1, starts.ctypes.data_as(DP), parents, replace, 0, None, C.byref(res_e)), "frirl_hip_batch_evolve_step")
                else:
                    frirl_amd.check(L.frirl_hip_batch_select(two, 1, starts.ctypes.data_as(DP), parents, replace, 0, None, None, C.byref(res_s)), "frirl_hip_batch_select")
                t = time.perf_counter() - t0
                if rnd:
                    (t_step if side == "e" else t_select).append(t)
            agree = agree and (res_e.best, res_e.replaced, res_e.rules_copied) == (res_s.best, res_s.replaced, res_s.rules_copied)
        out.update({"leg_same_result": agree, "replaced_last_round": int(res_e.replaced), "evolve_step": stats(t_step), "batch_select": stats(t_select)})
        out["leg_verdict"] = verdict(out["evolve_step"], out["batch_select"])
    finally:
        L.frirl_hip_batch_destroy(one)
        L.frirl_hip_batch_destroy(two)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", action="append", default=[])
    ap.add_argument("--agents", type=int, action="append", default=[])
    ap.add_argument("--max-rules", type=int, default=512)
    ap.add_argument("--episodes", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="markdown file to write the tables to")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [bench(env, E, a, dev) for env in (a.env or ["mountaincar", "acrobot"]) for E in (a.agents or [4096, 65536])]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# The selection leg on the device against through the host\n\n")
            f.write(f"`tools/evolve_bench.py`, {a.rounds} timed rounds after one warm-up, sides alternating; half of the agents replaced by the other half, n = 1; "
                    f"maxR = {a.max_rules}; the population: 64 start states, {a.episodes} episodes, tiled and shuffled over the batch.  Times are the minimum over the rounds, "
                    "spread = (max - min) / min.  `holds`: the device side is no slower than the host side by more than the larger of the two spreads (in us).\n\n")
            f.write("## (a) frirl_hip_select_plan_device (device events) against D2H scores + frirl_hip_select_plan + H2D src (host clock)\n\n")
            f.write("| env | agents | plan_device us (spread) | G pair tests / s | host leg us (spread) | host / device | margin us | holds | same src |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                p, h, v = r["plan_device"], r["plan_host_leg"], r["plan_verdict"]
                f.write(f"| {r['env']} | {r['agents']} | {p['min_us']} ({p['spread']}) | {p['pair_tests_per_s']} | {h['min_us']} ({h['spread']}) | {v['host_over_device']} | "
                        f"{v['margin_us']} | {v['holds']} | {r['plan_same_src']} |\n")
            f.write("\n## (b) frirl_hip_batch_evolve_step(spec = NULL) against frirl_hip_batch_select (host clock, twin batches)\n\n")
            f.write("| env | agents | evolve_step us (spread) | batch_select us (spread) | select / step | margin us | holds | same result |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                p, h, v = r["evolve_step"], r["batch_select"], r["leg_verdict"]
                f.write(f"| {r['env']} | {r['agents']} | {p['min_us']} ({p['spread']}) | {h['min_us']} ({h['spread']}) | {v['host_over_device']} | {v['margin_us']} | {v['holds']} | "
                        f"{r['leg_same_result']} |\n")
            f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
