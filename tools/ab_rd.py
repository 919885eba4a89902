#!/usr/bin/env python3
"""Interleaved A/B of distance-kernel variants in ONE process (frirl_hip_set_option between launches).
VARIANTS="nt,unroll,chunk[,persist[,order[,packed[,sqdiff[,qpass[,prepass[,coded]]]]]]];..."  (-1 / 0 = shipped value; packed: 1 = shipped, 0 = 16-bit
mirror; sqdiff: 1 = squared-difference tables (shipped), 0 = the packed scan without them; qpass: 1 = observation pre-pass of the
per-workgroup tables; prepass: 1 = tables built once per call in the workspace (shipped), 0 = per workgroup; coded: 1 = 3-byte lane-tiled codes where the
rule bases' dictionaries allow them (shipped), 0 = the 4-byte packed words)"""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, frirl_amd
import bench

w = dict(bench.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "cfg2_mountaincar_8k_x_8k"])
if len(sys.argv) > 2:
    w["E"] = int(sys.argv[2])
dev = torch.device("cuda", 0)
if w["env"]:
    prob, agent, envs = frirl_amd.demo_batch(w["env"], w["E"], w["R"], w["R"] + 256, dev, seed=0)
    del envs
else:
    prob, _, _ = bench.synth_problem(w, dev, 0)
x = bench.make_queries(prob, dev, 0)
dists = torch.empty((prob.E, prob.maxR), dtype=torch.float64, device=dev)
hit = torch.empty((prob.E,), dtype=torch.int32, device=dev)
variants = [tuple(map(int, v.split(","))) for v in os.environ.get("VARIANTS", "-1,0,0,-1,0;-1,0,0,-1,1;-1,0,0,0,0;-1,0,0,1,0;-1,0,4096,0,0;-1,0,1024,0,0").split(";")]
DEFAULTS = (-1, 0, 0, -1, 0, 1, 1, int(os.environ.get("FRIRL_HIP_RD_QPASS", "0")), int(os.environ.get("FRIRL_HIP_RD_PREPASS", "1")),
            int(os.environ.get("FRIRL_HIP_RD_CODED", "1")))
variants = [v + DEFAULTS[len(v):] for v in variants]
compressed = prob.uidx is not None and not os.environ.get("AB_F64")
if not compressed:
    prob = frirl_amd.Problem(prob.u, prob.ve, prob.rb, prob.nrules)
W = frirl_amd.lib().five_hip_rule_distance_packed_words(prob.nant, prob.U) if compressed else 0
alg = ((2.0 if compressed else 8.0) * prob.nant + 8.0) * prob.E * w["R"]      # bytes the 16-bit / f64 kernel moves (packed: 4 W + 8 per eval)
res = {v: [] for v in variants}
for rep in range(int(os.environ.get("REPS", "6"))):
    for v in variants:
        for name, val in zip(("rd_nt", "rd_unroll", "rd_chunk", "rd_persist", "rd_order", "rd_packed", "rd_sqdiff", "rd_qpass", "rd_prepass", "rd_coded"), v):
            frirl_amd.set_option(name, val)
        for _ in range(3):
            prob.rule_distance(x, ruledists=dists, hit=hit)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            prob.rule_distance(x, ruledists=dists, hit=hit)
        e1.record()
        torch.cuda.synchronize()
        res[v].append(e0.elapsed_time(e1) / 20)
for v in variants:
    t = sorted(res[v])
    med = t[len(t) // 2]
    moved = (4.0 * W + 8.0) * prob.E * w["R"] if (W and v[5] and v[3] != 1) else alg
    if W and v[9] and prob.codes is not None and v[5] and v[6] and v[8] and v[3] != 1 and v[4] == 0 and v[1] in (0, 4) and v[2] in (0, 2048):
        moved = (3.0 + 8.0) * prob.E * w["R"]
    print(f"nt={v[0]} unroll={v[1]} chunk={v[2]} persist={v[3]} order={v[4]} packed={v[5]} sqdiff={v[6]} qpass={v[7]} prepass={v[8]} coded={v[9]}: median {med:.4f} ms  min {t[0]:.4f}  -> {moved / med / 1e6:.0f} GB/s (median)")
