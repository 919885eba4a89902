#!/usr/bin/env python3
"""Records per second of learning a recorded demonstration, three ways, on fresh rule bases:
  (a) one frirl_hip_update_sarsa launch per record (the caller keeps the episode state: q_ant, cur_q_ant and the mask are prepared
      outside the timed window, so this side pays launches only)
  (b) the taught caller-stepped loop: frirl_hip_agent_begin_taught at the start records, frirl_hip_agent_observe_taught elsewhere
  (c) frirl_hip_learn_demonstration: the whole log in one launch
python tools/teach_bench.py [--env acrobot --env cartpole] [--agents 64 --agents 4096 --agents 65536] [--records 1000] [--rounds 3]
The logs are those of the scripted teachers (bang-bang on the acrobot's angular velocities, a clipped linear law on the cartpole, one
pick in ten random) stepped on the device with frirl_hip_env_step; every agent's episodes start together every --episode records, and
an agent whose episode ends early leaves records the three ways all skip.  The three sides alternate; round 0 warms up."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
import frirl_amd


def teacher(env, A, x, gen):
    if env == "acrobot":
        a = torch.where(x[:, 2] + x[:, 3] >= 0, 2, 0)
    elif env == "mountaincar":
        a = torch.where(x[:, 1] >= 0, 2, 0)
    else:
        a = torch.round(A // 2 + 10.0 * (0.1 * x[:, 0] + 0.3 * x[:, 1] + 6.0 * x[:, 2] + 0.9 * x[:, 3])).clamp(0, A - 1).long()
    rnd = torch.rand(x.shape[0], generator=gen, device=x.device)
    other = (torch.rand(x.shape[0], generator=gen, device=x.device) * A).long().clamp(0, A - 1)
    return torch.where(rnd < 0.1, other, a).to(torch.int32)


def record(env, d, E, T, episode, dev):
    """Logs [T, E, ...] (record-major, for the per-record ways), stepped with the demo's dynamics on the device."""
    agent = frirl_amd.demo_agent(d, dev, max_steps=episode - 1)
    ns, A = d["nstates"], d["A"]
    av = torch.from_numpy(d["grids"][-1]).to(dev)
    gen = torch.Generator(device=dev).manual_seed(17)
    vd = torch.tensor(d["values_def"][:ns], dtype=torch.float64, device=dev)
    obs, q_obs = torch.zeros((T, E, ns), dtype=torch.float64, device=dev), torch.zeros((T, E, ns), dtype=torch.float64, device=dev)
    action, success = torch.zeros((T, E), dtype=torch.int32, device=dev), torch.zeros((T, E), dtype=torch.int32, device=dev)
    reward, start = torch.zeros((T, E), dtype=torch.float64, device=dev), torch.zeros((T, E), dtype=torch.uint8, device=dev)
    x = None
    for r in range(T):
        if r % episode == 0:
            x = (vd + 0.02 * (torch.rand((E, ns), generator=gen, device=dev, dtype=torch.float64) - 0.5)).contiguous()
            start[r] = 1
        else:
            x, reward[r], success[r], q_obs[r] = frirl_amd.env_step(agent, av[action[r - 1].long()].contiguous(), x)
        obs[r] = x
        action[r] = teacher(env, A, x, gen)
    return dict(obs=obs, q_obs=q_obs, action=action, reward=reward, success=success, start=start)


def bench(env, E, a, dev):
    d = frirl_amd.demo_describe(env)
    nant, T = d["nant"], a.records
    log = record(env, d, E, T, a.episode, dev)
    prob, agent, envs = frirl_amd.fresh_batch(d, E, a.max_rules, dev, max_steps=a.episode - 1)
    state = (prob.rb, prob.nrules, prob.uidx, envs.rant, envs.states, envs.q_ant, envs.fus, envs.done, envs.ep_steps, envs.ep_reward, envs.status,
             envs.episode, envs.spread_ant, envs.spread_R)
    snap = [t.clone() for t in state]

    def restore():
        for t, t0 in zip(state, snap):
            t.copy_(t0)
        torch.cuda.synchronize()

    # (a): what the caller of frirl_hip_update_sarsa has to keep per record, prepared here
    av = torch.from_numpy(d["grids"][-1]).to(dev)
    aval = av[log["action"].long()]
    cur_q_ant = torch.cat([log["q_obs"], aval[..., None]], 2).contiguous()
    q_ant = torch.empty_like(cur_q_ant)
    q_ant[1:] = cur_q_ant[:-1]
    first = torch.cat([log["obs"], aval[..., None]], 2)
    q_ant[1:] = torch.where((log["start"][:-1] != 0)[..., None], first[:-1], q_ant[1:])       # the step after a start: the un-quantised start state
    active = torch.zeros((T, E), dtype=torch.uint8, device=dev)
    done = torch.zeros((E,), dtype=torch.bool, device=dev)
    steps = torch.zeros((E,), dtype=torch.int32, device=dev)
    for r in range(T):
        st = log["start"][r] != 0
        done, steps = done & ~st, torch.where(st, torch.zeros_like(steps), steps)
        act = ~st & ~done
        active[r] = act.to(torch.uint8)
        steps = steps + act.to(torch.int32)
        done = done | (act & ((log["success"][r] == 1) | (steps >= a.episode - 1)))
    # every agent starts its episodes at the same records here (record()), so agent 0's flag decides between begin and observe for the
    # whole batch; logs whose agents start at different records need the reset mask and a done mask per call (tests/test_hip_teach.py: chain)
    assert bool((log["start"] == log["start"][:, :1]).all())
    is_start = [bool(log["start"][r, 0]) for r in range(T)]
    # (c): agent-major copies
    demo = frirl_amd.Demonstration(*(log[k].transpose(0, 1).contiguous() for k in ("obs", "action", "reward", "success")),
                                   q_obs=log["q_obs"].transpose(0, 1).contiguous(), start=log["start"].transpose(0, 1).contiguous())
    torch.cuda.synchronize()

    def way_a():
        for r in range(T):
            if not is_start[r]:
                frirl_amd.update_sarsa(prob, agent, envs, q_ant[r], log["reward"][r], cur_q_ant[r], active=active[r])

    def way_b():
        for r in range(T):
            if is_start[r]:
                frirl_amd.agent_begin(prob, agent, envs, log["obs"][r], teacher=log["action"][r])
            else:
                frirl_amd.agent_observe(prob, agent, envs, log["obs"][r], log["reward"][r], log["success"][r], q_obs=log["q_obs"][r], teacher=log["action"][r])

    def way_c():
        frirl_amd.learn_demonstration(prob, agent, envs, demo)

    ways = {"update_sarsa_per_record": way_a, "taught_loop": way_b, "replay": way_c}
    times, rules = {k: [] for k in ways}, {}
    for rnd in range(a.rounds + 1):
        for k, fn in ways.items():
            restore()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                times[k].append(dt)
            rules[k] = prob.nrules.clone()
    same = all(torch.equal(rules["replay"], v) for v in rules.values())       # different rule counts = different work: main() fails on it
    learned = int(active.sum())
    out = {"env": env, "agents": E, "records": T, "records_learned_per_agent": learned / E, "rules_mean": float(rules["replay"].double().mean()),
           "rules_max": int(rules["replay"].max()), "same_rule_counts": same, "rules_sum": {k: int(v.sum()) for k, v in rules.items()}, "conclusions_per_rule_and_record": {"replay": 2, "taught_loop": d["A"] + 1}}
    for k, ts in times.items():
        out[k] = {"s": [round(t, 5) for t in ts], "records_per_s": E * T / min(ts), "spread": (max(ts) - min(ts)) / min(ts)}
    for k in ("update_sarsa_per_record", "taught_loop"):
        out["replay_over_" + k] = {"min_over_min": min(times[k]) / min(times["replay"]), "worst_case": min(times[k]) / max(times["replay"])}
    print(json.dumps(out), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", action="append", default=[])
    ap.add_argument("--agents", type=int, action="append", default=[])
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--episode", type=int, default=200, help="records per episode: every agent starts one together")
    ap.add_argument("--max-rules", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bad = []
    for env in (a.env or ["acrobot", "cartpole"]):
        for E in (a.agents or [64, 4096, 65536]):
            if not bench(env, E, a, dev):
                bad.append((env, E))
    if bad:
        raise SystemExit(f"the three ways ended with different rule counts (different work, the comparison does not hold) at {bad}")


if __name__ == "__main__":
    main()
