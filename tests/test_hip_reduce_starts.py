"""Reduction against a set of start states (frirl_hip_reduce_batch_starts, csrc/reduce_starts.hip): every removal of every agent's
reduction validated against several start states -- against the CPU model over the oracle (tests/reduce_starts_ref.py: the
reference's try-remove loop with the all-starts acceptance), against frirl_hip_reduce_batch for one start, and for the device state
it leaves behind.  The rule bases are those of tests/test_hip_reduce_batch.py (trained by the oracle, once per environment).

Arg-max ties: the comparisons are exact (same surviving rules, bit-equal, in the same order; same steps and rewards per start), so no
replay may differ from the oracle's at all; observed on an MI355X: 0 picks resolved differently in any case of this file."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import reduce_starts_ref as ref
from tests.test_dropin import write_bin
from tests.test_hip_reduce_batch import BatchDesc, Trained, agent_for, case, check_agent, device, spread_starts, upload

pytestmark = pytest.mark.gpu


def tens(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def starts_around(env, center, n, spread, seed):
    """n start states: row 0 = center, the others center +- spread * span (clipped) -- spread_starts' draw order around `center`"""
    probe = ob.Frirl(env, trig_mode=1)
    probe.set_start_state(center)                                    # dim(k)["values_def"] is the CURRENT start state
    return spread_starts(probe, n, spread, seed)


def run_starts(env, agents, starts, strategy, depth, count=None, drop=False, with_uidx=False, active=None):
    import torch
    prob, rant_d, host = upload(agents, with_uidx)
    act = None if active is None else tens(np.asarray(active, dtype=np.uint8))
    cnt = None if count is None else tens(np.asarray(count, dtype=np.int32))
    kept, res, per = prob.reduce_batch_starts(agent_for(env), strategy, 0.0, depth, tens(np.asarray(starts, dtype=np.float64)), start_count=cnt,
                                              drop_bad_starts=drop, rant=rant_d, active=act)
    torch.cuda.synchronize()
    return kept, res, per, prob, rant_d, host


def per_tuple(p):
    return (p.used, p.steps_incremental, p.baseline_reward, p.reward)


def depth_used(depth, E, n, A=3):
    return depth or frirl_amd.lib().frirl_hip_reduce_batch_starts_depth(E, A, n)


def check_against_model(a, want, kept, res, per, depth, count):
    """agent `a` after a call against the model's Outcome `want`: surviving rules bit-equal and in the model's order, per-start results,
    the counters"""
    assert list(kept) == want.kept, (len(kept), len(want.kept))
    assert [per_tuple(p) for p in per] == want.per_start
    assert (res.rules_before, res.rules_after) == (a.R0, len(want.kept))
    assert (res.steps_incremental, res.reward) == want.first()
    assert (res.rounds, res.rollouts) == ref.counters(a.R0, depth, count, len(want.used))


def result_fields(r):
    return (r.rules_before, r.rules_after, r.rounds, r.rollouts, r.steps_incremental, r.reserved, r.reward)


# ---- 1. one start state: frirl_hip_reduce_batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,depth", [(1, 0), (2, 3)])
def test_one_start_equals_reduce_batch(strategy, depth):
    """n = 1, drop_bad_starts = 0: kept, every result field and the device state (rb, rant, uidx, nrules) of Problem.reduce_batch"""
    import torch
    agents = case("mountaincar")[:3]
    start = np.stack([a.start for a in agents])
    prob0, rant0, _ = upload(agents, True)
    kept0, res0 = prob0.reduce_batch(agent_for("mountaincar"), strategy, 0.0, depth, rant=rant0, start_states=tens(start))
    torch.cuda.synchronize()
    kept, res, per, prob, rant_d, host = run_starts("mountaincar", agents, start[:, None, :], strategy, depth, with_uidx=True)
    assert [r.rules_after for r in res] == {1: [28, 25, 23], 2: [52, 31, 26]}[strategy]
    for e in range(3):
        assert (kept[e] == kept0[e]).all() and result_fields(res[e]) == result_fields(res0[e]), e
        assert per_tuple(per[e][0]) == (1, res0[e].steps_incremental, agents[e].baseline()[1], res0[e].reward)
        check_agent("mountaincar", agents, e, strategy, depth_used(depth, 3, 1), kept[e], res[e], prob, rant_d, host, True)
    for x, y in ((prob.rb, prob0.rb), (rant_d, rant0), (prob.uidx, prob0.uidx), (prob.nrules, prob0.nrules)):
        assert (x.cpu().numpy() == y.cpu().numpy()).all()


# ---- 2. several starts, ragged ---------------------------------------------------------------------------------------------------------
RAGGED_COUNT = [3, 1, 2]


@functools.lru_cache(maxsize=None)
def ragged_starts():
    """three starts per agent at spread 0.4 around the agent's own; the baselines of the agents' rule bases run 24 ... 472 steps there,
    so rows with very different caps share a workgroup"""
    return np.stack([starts_around("mountaincar", a.start, 3, 0.4, 21 + e) for e, a in enumerate(case("mountaincar")[:3])])


@functools.lru_cache(maxsize=None)
def ragged_model(e, strategy):
    return ref.sequential(case("mountaincar")[e], ragged_starts()[e], strategy, count=RAGGED_COUNT[e])


@pytest.mark.parametrize("strategy,with_uidx", [(1, True), (2, False)])
def test_ragged_starts_equal_the_model_at_every_depth(strategy, with_uidx):
    """E = 3, n = 3, start_count = [3, 1, 2]; depths 0, 3 and 1 keep identical sets (invariance)"""
    agents = case("mountaincar")[:3]
    starts = ragged_starts()
    want = [ragged_model(e, strategy) for e in range(3)]
    assert [len(w.kept) for w in want] == {1: [28, 25, 23], 2: [53, 31, 27]}[strategy]
    caps = [p[1] for w in want for p in w.per_start if p[0]]
    assert min(caps) < 100 and max(caps) > 400, caps
    first = None
    for depth in (0, 3, 1):
        kept, res, per, prob, rant_d, host = run_starts("mountaincar", agents, starts, strategy, depth, count=RAGGED_COUNT, with_uidx=with_uidx)
        d = depth_used(depth, 3, 3)
        for e in range(3):
            check_against_model(agents[e], want[e], kept[e], res[e], per[e], d, RAGGED_COUNT[e])
            check_agent(None, agents, e, strategy, d, kept[e], res[e], prob, rant_d, host, with_uidx, oracle=False)
        if first is None:
            first = kept
        assert all((k == k0).all() for k, k0 in zip(kept, first)), depth


def test_inactive_agent_is_untouched():
    agents = case("mountaincar")[:3]
    kept, res, per, prob, rant_d, host = run_starts("mountaincar", agents, ragged_starts(), 1, 3, count=RAGGED_COUNT, with_uidx=True, active=[1, 0, 1])
    rb0, rant0, uidx0 = host
    for e in (0, 2):
        check_against_model(agents[e], ragged_model(e, 1), kept[e], res[e], per[e], 3, RAGGED_COUNT[e])
        check_agent(None, agents, e, 1, 3, kept[e], res[e], prob, rant_d, host, True, oracle=False)
    assert (prob.rb[1].cpu().numpy() == rb0[1]).all() and (rant_d[1].cpu().numpy() == rant0[1]).all() and (prob.uidx[1].cpu().numpy() == uidx0[1]).all()
    assert int(prob.nrules[1]) == agents[1].R0 == res[1].rules_before == res[1].rules_after
    assert res[1].rounds == 0 and res[1].rollouts == 0 and (kept[1] == np.arange(agents[1].R0)).all()
    assert [per_tuple(p) for p in per[1]] == [(0, -1, 0.0, 0.0)] * 3


# ---- 3. start states whose baseline episode is not good ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def acrobot_starts():
    """per agent (the first two of case("acrobot")): the good and the bad ones among 64 start states at spread 0.05, by the oracle"""
    probe = ob.Frirl("acrobot", trig_mode=1)
    cand = spread_starts(probe, 64, 0.05)
    out = []
    for a in case("acrobot")[:2]:
        rp = ref.Replayer(a)
        good = [rp.replay(list(range(a.R0)), s)[1] > rp.good_above for s in cand]
        out.append((cand[[i for i in range(64) if good[i]]], cand[[i for i in range(64) if not good[i]]]))
        assert len(out[-1][0]) >= 2 and len(out[-1][1]) >= 4
    return out


def mixed_starts():
    """n = 4: good, bad, good, bad for both agents"""
    return np.stack([np.stack([g[0], b[0], g[1], b[1]]) for g, b in acrobot_starts()])


@functools.lru_cache(maxsize=None)
def acrobot_model(e):
    return ref.sequential(case("acrobot")[e], mixed_starts()[e], 1, drop_bad_starts=True)


def test_bad_starts_block_every_removal_when_they_stay_in():
    agents = case("acrobot")[:2]
    kept, res, per, prob, rant_d, host = run_starts("acrobot", agents, mixed_starts(), 1, 5)
    for e, a in enumerate(agents):
        assert res[e].rules_after == a.R0 and (kept[e] == np.arange(a.R0)).all() and res[e].rounds == -(-a.R0 // 5)
        assert [p.used for p in per[e]] == [1, 1, 1, 1] and res[e].rollouts == 4 + 4 * sum(2 ** min(5, a.R0 - j) - 1 for j in range(0, a.R0, 5))
        want = acrobot_model(e).per_start
        assert [per_tuple(p)[1:] for p in per[e]] == [(w[1], w[2], w[2]) for w in want]      # the baselines; no removal, so reward stays
        check_agent(None, agents, e, 1, 5, kept[e], res[e], prob, rant_d, host, False, oracle=False)


def test_bad_starts_are_dropped_on_the_device():
    agents = case("acrobot")[:2]
    kept, res, per, prob, rant_d, host = run_starts("acrobot", agents, mixed_starts(), 1, 0, drop=True)
    d = depth_used(0, 2, 4)
    for e, a in enumerate(agents):
        want = acrobot_model(e)
        assert want.used == [0, 2] and len(want.kept) < a.R0
        check_against_model(a, want, kept[e], res[e], per[e], d, 4)
        check_agent(None, agents, e, 1, d, kept[e], res[e], prob, rant_d, host, False, oracle=False)
    assert [len(acrobot_model(e).kept) for e in range(2)] == [225, 72]


def test_agent_with_only_bad_starts_finishes_after_the_baseline():
    agents = case("acrobot")[:2]
    (g0, b0), (g1, b1) = acrobot_starts()
    starts = np.stack([np.stack([g0[0], b0[0], g0[1], b0[1]]), b1[:4]])
    kept, res, per, prob, rant_d, host = run_starts("acrobot", agents, starts, 1, 6, drop=True)
    check_against_model(agents[0], acrobot_model(0), kept[0], res[0], per[0], 6, 4)
    a = agents[1]
    assert (res[1].rules_before, res[1].rules_after, res[1].rounds, res[1].rollouts) == (a.R0, a.R0, 0, 4) and (kept[1] == np.arange(a.R0)).all()
    assert [p.used for p in per[1]] == [0, 0, 0, 0] and all(p.steps_incremental > 0 and p.reward == p.baseline_reward for p in per[1])
    assert (res[1].steps_incremental, res[1].reward) == (per[1][0].steps_incremental, per[1][0].reward)          # start 0 where none is used
    rb0, rant0, _ = host
    assert (prob.rb[1].cpu().numpy() == rb0[1]).all() and (rant_d[1].cpu().numpy() == rant0[1]).all() and int(prob.nrules[1]) == a.R0


# ---- 4. 21 actions ---------------------------------------------------------------------------------------------------------------------
def test_cartpole_one_rule_base_two_start_states():
    """21 actions (8 lanes per row, three passes of 4 conclusions): the default rule base validated against the two start states of
    tests/test_hip_reduce_batch.py's cartpole case, whose baseline episodes differ"""
    first, second = case("cartpole")
    assert first.baseline() != second.baseline()
    starts = np.stack([first.start, second.start])[None]
    want = ref.sequential(first, starts[0], 1)
    kept, res, per, prob, rant_d, host = run_starts("cartpole", [first], starts, 1, 0)
    d = depth_used(0, 1, 2, 21)
    check_against_model(first, want, kept[0], res[0], per[0], d, 2)
    check_agent(None, [first], 0, 1, d, kept[0], res[0], prob, rant_d, host, False, oracle=False)
    assert per[0][0].steps_incremental != per[0][1].steps_incremental or per[0][0].baseline_reward != per[0][1].baseline_reward
    assert len(want.kept) == 40                                       # 7 with the default start state alone


# ---- 5. the batch object and the demo ------------------------------------------------------------------------------------------------------
def test_batch_object_reduces_every_agent_against_its_start_states():
    """frirl_hip_batch_reduce_all_starts: three mountaincar agents trained on the device from desc.start_states, n = 2 (the agent's own
    start and one at spread 0.4 around it), against the model run on each agent's learned rule base (downloaded before the reduction)."""
    L = frirl_amd.lib()
    d = frirl_amd.demo_describe("mountaincar")
    nant, E, maxR, n = d["nant"], 3, 512, 2
    own = np.ascontiguousarray(np.stack([a.start for a in case("mountaincar")[:E]]))
    starts = np.ascontiguousarray(np.stack([starts_around("mountaincar", own[e], n, 0.4, 31 + e) for e in range(E)]))
    grid = np.zeros((nant, frirl_amd.MAX_GRID))
    for k, g in enumerate(d["grids"]):
        grid[k, : len(g)] = g
    ncorner = 2 ** nant
    rant0 = np.zeros((ncorner, nant))
    for k in range(nant):
        div = ncorner >> (k + 1)
        rant0[:, k] = [d["grids"][k].min() if ((j // div) % 2) == 0 else d["grids"][k].max() for j in range(ncorner)]
    rconc0 = np.zeros(ncorner)
    u, ve, ave = np.ascontiguousarray(d["u"]), np.ascontiguousarray(d["ve"]), np.ascontiguousarray(d["action_ve"])
    desc = BatchDesc()
    desc.nant, desc.U, desc.E, desc.maxR, desc.u, desc.ve = nant, d["U"], E, maxR, u.ctypes.data, ve.ctypes.data
    desc.R0, desc.rant0, desc.rconc0, desc.start_states = ncorner, rant0.ctypes.data, rconc0.ctypes.data, own.ctypes.data
    ag = desc.agent
    ag.alpha, ag.gamma, ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"]
    ag.weight_significant, ag.skip_rules, ag.A, ag.env_kind, ag.max_steps, ag.no_random = d["weight_thr"], d["skip_rules"], d["A"], d["kind"], d["max_steps"], 1
    ag.reward_good_above, ag.qdiff_final_tolerance = d["reward_good_above"], d["qdiff_final_tolerance"]
    for k in range(nant):
        ag.grid_len[k], ag.grid_div[k], ag.values_def[k] = len(d["grids"][k]), d["grid_div"][k], d["values_def"][k]
    ag.grid_values, ag.action_ve = grid.ctypes.data, ave.ctypes.data
    b = L.frirl_hip_batch_create(C.byref(desc))
    assert b, L.frirl_hip_last_error()
    dp = C.POINTER(C.c_double)
    try:
        episodes = C.c_int32()
        frirl_amd.check(L.frirl_hip_batch_train(b, 1000, C.byref(episodes)), "frirl_hip_batch_train")

        def download(e):
            R = C.c_int32()
            rant, rconc = np.zeros((maxR, nant)), np.zeros(maxR)
            frirl_amd.check(L.frirl_hip_batch_get_rulebase(b, e, C.byref(R), rant.ctypes.data_as(dp), rconc.ctypes.data_as(dp)), "frirl_hip_batch_get_rulebase")
            return rant[: R.value].copy(), rconc[: R.value].copy()

        before = [download(e) for e in range(E)]
        res = (frirl_amd.ReduceResult * E)()
        per = (frirl_amd.ReduceStartResult * (E * n))()
        reduced = C.c_int32(-1)
        for bad_n in (0, 257):
            assert L.frirl_hip_batch_reduce_all_starts(b, 1, 0.0, 0, bad_n, starts.ctypes.data_as(dp), 1, res, per, C.byref(reduced)) == -2
        assert L.frirl_hip_batch_reduce_all_starts(b, 1, 0.0, 0, n, None, 1, res, per, C.byref(reduced)) == -2 and reduced.value == -1
        frirl_amd.check(L.frirl_hip_batch_reduce_all_starts(b, 1, 0.0, 0, n, starts.ctypes.data_as(dp), 1, res, per, C.byref(reduced)),
                        "frirl_hip_batch_reduce_all_starts")
        assert reduced.value == sum(r.rules_after < r.rules_before for r in res) > 0
        for e in range(E):
            rant, rconc = download(e)
            t = Trained("mountaincar", own[e], rules=before[e])
            want = ref.sequential(t, starts[e], 1, drop_bad_starts=True)
            assert res[e].rules_before == t.R0 and res[e].rules_after == len(rconc) == len(want.kept), (e, len(rconc), len(want.kept))
            assert (rant == t.rant[want.kept]).all() and (rconc == t.rconc[want.kept]).all(), f"agent {e}"
            assert [per_tuple(per[e * n + k]) for k in range(n)] == want.per_start
    finally:
        L.frirl_hip_batch_destroy(b)


def test_demo_with_one_start_and_no_spread_is_the_run_without_the_flag(tmp_path):
    """`--reduce-starts 1 --spread 0`: stdout, the saved rule bases and the dumped rule base byte-equal to the run without the flag"""
    frirl_amd.build()
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    a = case("mountaincar")[0]
    outs = []
    for name, extra in (("plain", []), ("starts", ["--reduce-starts", "1", "--spread", "0"])):
        work = tmp_path / name
        work.mkdir()
        write_bin(work / "one.bin", [(a.rant, a.rconc)])
        r = subprocess.run([demo, "--env", "mountaincar", "--agents", "3", "--load", "one.bin", "--save", "all.bin", "--reduce", "1", "--reduce-all"] + extra,
                           cwd=work, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append((r.stdout, (work / "all.bin").read_bytes(), (work / "mountaincar.batch.reduced1.frirlrb.txt").read_bytes()))
    assert outs[0] == outs[1]
    assert b"3 of 3 agents reduced, 330 -> 84 rules" in outs[0][0], outs[0][0][-600:]
    # several start states: the summary line says how many were used
    work = tmp_path / "four"
    work.mkdir()
    write_bin(work / "one.bin", [(a.rant, a.rconc)])
    r = subprocess.run([demo, "--env", "mountaincar", "--agents", "3", "--load", "one.bin", "--reduce", "1", "--reduce-all", "--reduce-starts", "4",
                        "--spread", "0.3"], cwd=work, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and re.search(r"agents reduced, 330 -> \d+ rules \(.*\), starts used \d+ of 12\n", r.stdout), r.stdout[-600:] + r.stderr[-600:]
