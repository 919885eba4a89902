#!/usr/bin/env python3
"""Time of replacing half of a trained population by copies of the other half, two ways, on the same tensors:
  (a) frirl_hip_clone_agents: one call (the copy launch and the scalar launch)
  (b) what a caller can do without it: torch index copies x[dst] = x[src_idx] over the same arrays, whole maxR slabs, one launch or
      more per array
python tools/select_bench.py [--env mountaincar --env acrobot] [--agents 4096 --agents 65536] [--rounds 5] [--out profiles/r27_select.md]
The population: 64 agents with start states spread over the state grids train --episodes episodes (the persistent learner), and agent e
of the measured batch is a copy of trained agent e mod 64, so the rule counts are those of real learners.  Agent e >= E / 2 takes agent
e - E / 2.  Before every timed call the destinations' rule counts are put back (the columns moved depend on them); the sides alternate,
round 0 warms up, each round is timed with device events around the calls of one side.  Bytes per launch are counted from the contract
of include/frirl_hip.h: per cloned agent and copied row the source's columns read plus max(old, new) columns written."""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
import frirl_amd

PEAK_TBS = 8.0


def population(env, E, a, dev):
    d = frirl_amd.demo_describe(env)
    E0 = min(64, E)
    rng = np.random.default_rng(11)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E0) for k in range(d["nstates"])], 1))).to(dev)
    p0, agent, e0 = frirl_amd.demo_fresh_batch(env, E0, a.max_rules, dev, start_states=start)
    c0 = frirl_amd.train_persistent(p0, agent, e0, max_episodes=a.episodes[env] + 1).conv
    torch.cuda.synchronize()
    pick = torch.arange(E, device=dev) % E0
    # trained agents in shuffled order, so that a destination and its source hold different rule counts
    pick = pick[torch.from_numpy(rng.permutation(E)).to(dev)]
    prob = frirl_amd.Problem(p0.u, p0.ve, p0.rb[pick].contiguous(), p0.nrules[pick].contiguous(), uidx=p0.uidx[pick].contiguous())
    envs = frirl_amd.Envs(prob, dev, rant_init=e0.rant[pick].contiguous())
    conv = frirl_amd.Convergence(prob, dev)
    for k in ("fus", "spread_ant", "spread_R"):
        getattr(envs, k).copy_(getattr(e0, k)[pick])
    for k in ("prev_nrules", "prev_steps", "prev_reward", "prev_rconc", "converged", "episodes"):
        getattr(conv, k).copy_(getattr(c0, k)[pick])
    torch.cuda.synchronize()
    return d, prob, envs, conv


def bench(env, E, a, dev):
    d, prob, envs, conv = population(env, E, a, dev)
    nant, M = prob.nant, prob.maxR
    half = E // 2
    src = torch.arange(E, dtype=torch.int32, device=dev)
    src[half:] -= half
    dst = torch.arange(half, E, device=dev)
    sidx = src[half:].long()
    nr0, pn0 = prob.nrules.clone(), conv.prev_nrules.clone()
    nr = nr0.cpu().numpy().astype(np.int64)
    pn = pn0.cpu().numpy().astype(np.int64)
    ns, old, oldp = nr[: E - half], nr[half:], pn[half:]
    cols = np.maximum(old, ns)
    colsp = np.maximum(cols, oldp)
    rows8 = (nant + 1) + nant                                       # rb and rant rows, 8 bytes a column
    contract_bytes = int((8 * rows8 * (ns + cols) + 2 * nant * (ns + cols) + 8 * (ns + colsp)).sum())
    slab_bytes = int(2 * (E - half) * M * (8 * rows8 + 2 * nant + 8))     # what the index copies move: whole slabs read and written

    def restore():
        prob.nrules.copy_(nr0)
        conv.prev_nrules.copy_(pn0)

    def way_clone():
        prob.clone_agents(envs, src, conv=conv)

    def way_torch():
        prob.rb[dst] = prob.rb[sidx]
        envs.rant[dst] = envs.rant[sidx]
        prob.uidx[dst] = prob.uidx[sidx]
        conv.prev_rconc[dst] = prob.rb[sidx, nant]
        prob.nrules[dst] = prob.nrules[sidx]
        envs.fus[dst] = envs.fus[sidx]
        envs.spread_ant[dst] = envs.spread_ant[sidx]
        envs.spread_R[dst] = envs.spread_R[sidx]
        conv.prev_nrules[dst] = prob.nrules[sidx]
        conv.prev_steps[dst] = -1
        conv.prev_reward[dst] = -1.0
        conv.converged[dst] = 0
        conv.epended[dst] = 0

    ways = {"clone_agents": way_clone, "torch_index_copies": way_torch}
    times = {k: [] for k in ways}
    for rnd in range(a.rounds + 1):
        for k, fn in ways.items():
            restore()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                times[k].append(t0.elapsed_time(t1) * 1e-3)
    out = {"env": env, "agents": E, "cloned": E - half, "maxR": M, "rules_mean": float(nr.mean()), "rules_max": int(nr.max()),
           "contract_bytes": contract_bytes, "slab_bytes": slab_bytes}
    for k, ts in times.items():
        best = min(ts)
        out[k] = {"us": [round(t * 1e6, 1) for t in ts], "min_us": round(best * 1e6, 1), "spread": round((max(ts) - best) / best, 3)}
    t = min(times["clone_agents"])
    out["clone_agents"]["TB_per_s"] = round(contract_bytes / t / 1e12, 3)
    out["clone_agents"]["of_peak"] = round(contract_bytes / t / 1e12 / PEAK_TBS, 3)
    out["torch_index_copies"]["TB_per_s_of_slabs"] = round(slab_bytes / min(times["torch_index_copies"]) / 1e12, 3)
    out["torch_over_clone"] = {"min_over_min": round(min(times["torch_index_copies"]) / t, 2), "worst_case": round(min(times["torch_index_copies"]) / max(times["clone_agents"]), 2)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", action="append", default=[])
    ap.add_argument("--agents", type=int, action="append", default=[])
    ap.add_argument("--max-rules", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="markdown file to write the table to")
    a = ap.parse_args()
    a.episodes = {"mountaincar": 30, "acrobot": 30, "cartpole": 30}
    dev = torch.device("cuda:0")
    rows = [bench(env, E, a, dev) for env in (a.env or ["mountaincar", "acrobot"]) for E in (a.agents or [4096, 65536])]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# frirl_hip_clone_agents against torch index copies\n\n")
            f.write(f"`tools/select_bench.py`, {a.rounds} timed rounds after one warm-up, sides alternating, device events; half of the agents replaced; "
                    f"maxR = {a.max_rules}; the population: 64 agents trained 30 episodes from spread start states, tiled and shuffled.  Times are the minimum, spread = (max - min) / min over the rounds.  "
                    "Contract bytes: source columns read + max(old, new) columns written over rb, rant, uidx, prev_rconc.\n\n")
            f.write("| env | agents | rules mean / max | clone_agents us (spread) | contract MB | TB/s | of 8 TB/s | torch index copies us (spread) | slab MB | torch / clone |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                c, t = r["clone_agents"], r["torch_index_copies"]
                f.write(f"| {r['env']} | {r['agents']} | {r['rules_mean']:.1f} / {r['rules_max']} | {c['min_us']} ({c['spread']}) | {r['contract_bytes'] / 1e6:.1f} | "
                        f"{c['TB_per_s']} | {c['of_peak']} | {t['min_us']} ({t['spread']}) | {r['slab_bytes'] / 1e6:.1f} | {r['torch_over_clone']['min_over_min']} |\n")
            f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
