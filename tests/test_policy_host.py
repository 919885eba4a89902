"""Host side of the caller-stepped shared-rule-base API (no GPU needed): the new ABI symbols and struct layout, the argument checks
of frirl_hip_policy_begin / _observe and frirl_hip_reducer_create (EINVAL before ENODEV), and the checker the GPU tests use -- a
Python restatement of the sequential reduction loop (frirl_sequential_run.c:170-350) over ANY environment function -- pinned against
the oracle's own reduction (orc_reduce_run) on mountaincar."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob

NEW_SYMBOLS = ["frirl_hip_policy_begin", "frirl_hip_policy_observe", "frirl_hip_reducer_create", "frirl_hip_reducer_next_round",
               "frirl_hip_reducer_begin", "frirl_hip_reducer_observe", "frirl_hip_reducer_end_round", "frirl_hip_reducer_result",
               "frirl_hip_reducer_destroy"]


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


# ---- the pinned checker ---------------------------------------------------------------------------------------------------
class SequentialReduction:
    """frirl_sequential_run.c:170-350 with one candidate per replayed episode, built from the oracle's FIVE pieces
    (Five.best_action, Five.remove_rule) and an environment function env_fn(states, action value) -> (new states, reward, success,
    quantised new states).  The replay is frirl_episode with reduction_state == 1 (frirl_episode.c:28-194 without the update).

    device_pick(candidate number or -1 for the baseline, accepted-bits of the candidate's round so far, step) -> the device's action
    index or None.  Where the oracle's conclusions tie the device's pick within 1e-12 relative the device's pick is followed (as
    Mirror.pick of tests/test_hip_external.py: tie-breaking below the 1e-6 contract is not part of it) and counted in `ties`;
    `near_ties` counts the greedy picks whose runner-up is that close, whatever the device did."""

    def __init__(self, u, ve, rant, rconc, action_ve, action_values, start, env_fn, max_steps, reward_good_above, device_pick=None,
                 depth=10, p=0):
        self.u, self.ve = np.array(u), np.array(ve)
        self.nant, self.U = self.u.shape
        self.rant0, self.rconc0 = np.array(rant, dtype=np.float64), np.array(rconc, dtype=np.float64)
        self.action_ve, self.action_values = np.array(action_ve), np.array(action_values)
        self.start, self.env_fn, self.max_steps, self.good_above = np.array(start, dtype=np.float64), env_fn, max_steps, reward_good_above
        self.device_pick, self.depth, self.p = device_pick, depth, p          # p: Shepard power of every rule base it builds (0 = nant)
        self.ties = self.near_ties = self.picks = 0

    def five(self, alive):
        return ob.Five(self.u, self.ve, self.nant, self.U, len(self.rconc0) + 8, rant=self.rant0[alive], rconc=self.rconc0[alive], p=self.p)

    def pick(self, f, states, key, step):
        best, oc = f.best_action(states, self.action_ve)
        self.picks += 1
        others = np.delete(oc, best)
        if len(others) and np.any(np.abs(others - oc[best]) <= 1e-12 * abs(oc[best])):
            self.near_ties += 1
        dev = self.device_pick(key[0], key[1], step) if self.device_pick is not None else None
        if dev is not None and dev != best and abs(oc[dev] - oc[best]) <= 1e-12 * abs(oc[best]):
            self.ties += 1
            return int(dev)
        return best

    def replay(self, f, cap, key):
        states = self.start.copy()
        a = self.pick(f, states, key, 0)                                        # frirl_episode.c:78, un-quantised
        steps, total = 0, 0.0
        while True:
            states, r, success, q = self.env_fn(states, self.action_values[a])   # :97-112
            total += r                                                          # :107
            a = self.pick(f, q, key, steps + 1)                                 # :148
            steps += 1                                                          # :174
            if success == 1 or steps >= cap:                                    # :183, :86
                return steps, total

    def run(self, strategy, reward_tolerance=0.0):
        R0 = len(self.rconc0)
        alive = list(range(R0))
        steps_inc, prev_reward = self.replay(self.five(alive), self.max_steps, (-1, 0))     # :196-198
        order = np.argsort(np.abs(self.rconc0) if strategy == 1 else -np.abs(self.rconc0), kind="stable")   # :268 / :286
        bits = 0
        for i, c in enumerate(order):
            if i % self.depth == 0:
                bits = 0
            f = self.five(alive)
            f.remove_rule(alive.index(int(c)))                                  # five_remove_rule keeps the relative order
            steps, reward = self.replay(f, min(self.max_steps, steps_inc + 1), (i, bits))
            if reward > self.good_above and steps == steps_inc and abs(prev_reward - reward) <= reward_tolerance:   # :212
                alive.remove(int(c))
                prev_reward = reward                                            # :222
                bits |= 1 << (i % self.depth)
        self.steps_incremental, self.reward = steps_inc, prev_reward
        return alive


@pytest.mark.parametrize("strategy", [1, 2])
def test_python_sequential_loop_equals_oracle_reduction(strategy):
    fr = ob.Frirl("mountaincar", trig_mode=1)
    assert fr.run() == 1
    f = fr.five
    R0 = f.R
    rant0, rconc0 = np.array(f.rant[:R0]), np.array(f.rconc[:R0])
    start = [fr.dim(k)["values_def"] for k in range(fr.nstates)]

    def env_fn(states, action):
        ns, r, success, q = fr.env_step(action, states)
        return ns, r, success, q

    seq = SequentialReduction(f.u, f.ve, rant0, rconc0, fr.action_vevalues, fr.dim(fr.nstates)["values"], start, env_fn, 1000,
                              fr.hparams["reward_good_above"])
    kept = seq.run(strategy)
    fr.reduce(strategy, 0.0)
    assert 0 < f.R < R0 and f.R == len(kept)
    assert (np.array(f.rant[: f.R]) == rant0[kept]).all() and (np.array(f.rconc[: f.R]) == rconc0[kept]).all()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported(lib):
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    P = frirl_amd.PolicyRowsDesc
    assert C.sizeof(P) == 56 and P.done.offset == 8 and P.ep_steps.offset == 16 and P.success.offset == 24 and P.ep_reward.offset == 32
    assert P.exclude_mask.offset == 40 and P.rule_slot.offset == 48
    for name in ("policy_group", "policy_slices"):
        v = C.c_int(-7)
        assert lib.frirl_hip_get_option(name.encode(), C.byref(v)) == 0 and v.value == 0


def _valid_call(nant, A, E=1):
    buf = (C.c_double * 16384)()
    addr = (C.addressof(buf) + 15) & ~15
    t = frirl_amd.Tables(nant, 41, addr, addr)
    b = frirl_amd.RuleBases(E, 8, addr, addr)
    ag = frirl_amd.AgentDesc()
    ag.A, ag.env_kind, ag.max_steps, ag.grid_values, ag.action_ve = A, frirl_amd.ENV_EXTERNAL, 10, addr, addr
    for k in range(min(nant, frirl_amd.MAX_NANT)):
        ag.grid_len[k] = 3
    if 1 <= nant <= frirl_amd.MAX_NANT:
        ag.grid_len[nant - 1] = min(A, frirl_amd.MAX_GRID)
    rows = frirl_amd.PolicyRowsDesc(4, addr, addr, addr, addr, None, None)
    io = frirl_amd.AgentIO(addr, None, addr, addr, None, addr, None)
    return buf, t, b, ag, rows, io


def _both(lib, t, b, ag, rows, io):
    args = [C.byref(x) if x is not None else None for x in (t, b, ag, rows, io)] + [None]
    return lib.frirl_hip_policy_begin(*args), lib.frirl_hip_policy_observe(*args)


def test_policy_argument_checks_before_the_device(lib):
    import torch
    cases = []

    def case(what, nant=4, A=5, E=1):
        keep, t, b, ag, rows, io = _valid_call(nant, A, E)
        cases.append((what, [keep, t, b, ag, rows, io]))
        return cases[-1][1]

    case(b"E == 1", E=2)
    case(b"nant", nant=1)
    case(b"nant", nant=9)
    case(b"A=33", A=33)
    case(b"A=0", A=0)
    case(b"grid_len")[3].grid_len[1] = 0
    case(b"grid_len")[3].grid_len[0] = 65
    case(b"action grid")[3].grid_len[3] = 4
    case(b"row state")[4].done = None
    case(b"row state")[4].ep_steps = None
    case(b"row state")[4].success = None
    case(b"row state")[4].ep_reward = None
    case(b"Q=0")[4].Q = 0
    c = case(b"go together")
    c[4].exclude_mask = c[2].rb
    c = case(b"go together")
    c[4].rule_slot = c[2].rb
    case(b"NULL")[5].obs = None
    case(b"NULL")[5].action_out = None
    case(b"NULL")[3].grid_values = None
    case(b"NULL")[3].action_ve = None
    for what, (keep, t, b, ag, rows, io) in cases:
        rb, ro = _both(lib, t, b, ag, rows, io)
        assert ro == -2 and what in lib.frirl_hip_last_error(), (what, lib.frirl_hip_last_error())
        assert rb == -2, what
    # observe alone needs the reward and the success flag
    for field in ("reward", "success"):
        keep, t, b, ag, rows, io = _valid_call(4, 5)
        setattr(io, field, None)
        args = [C.byref(x) for x in (t, b, ag, rows, io)] + [None]
        assert lib.frirl_hip_policy_observe(*args) == -2 and b"reward" in lib.frirl_hip_last_error()
        if not torch.cuda.is_available():       # begin does not read them (never launched from here with these host addresses)
            assert lib.frirl_hip_policy_begin(*args) == -1
    keep, t, b, ag, rows, io = _valid_call(4, 5)
    assert _both(lib, t, b, None, rows, io) == (-2, -2) and _both(lib, t, b, ag, None, io) == (-2, -2) and _both(lib, t, b, ag, rows, None) == (-2, -2)
    if not torch.cuda.is_available():       # valid arguments: no CPU fallback, the device check answers
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, rows, io = _valid_call(nant, A)
            assert _both(lib, t, b, ag, rows, io) == (-1, -1)
            assert b"no CPU fallback" in lib.frirl_hip_last_error()
            rows.exclude_mask = rows.rule_slot = b.rb
            assert _both(lib, t, b, ag, rows, io) == (-1, -1)


def test_reducer_create_argument_checks(lib):
    import torch
    create = lib.frirl_hip_reducer_create

    def make(strategy=1, depth=0, nant=4, A=5, E=1):
        keep, t, b, ag, rows, io = _valid_call(nant, A, E)
        return create(C.byref(t), C.byref(b), C.byref(ag), None, strategy, 0.0, depth, None)

    for kw, what in ((dict(strategy=0), b"strategy 0"), (dict(strategy=3), b"strategy 3"), (dict(depth=13), b"depth 13"), (dict(depth=-1), b"depth"),
                     (dict(E=2), b"E == 1"), (dict(nant=9), b"nant"), (dict(A=33), b"A=33")):
        assert make(**kw) is None
        assert what in lib.frirl_hip_last_error(), (kw, lib.frirl_hip_last_error())
    if not torch.cuda.is_available():
        for depth in (0, 1, 12):
            assert make(depth=depth) is None and b"no CPU fallback" in lib.frirl_hip_last_error()
    # the other calls refuse a NULL handle
    q = C.c_int32()
    res = frirl_amd.ReduceResult()
    assert lib.frirl_hip_reducer_next_round(None, C.byref(q)) == -2 and lib.frirl_hip_reducer_begin(None, None) == -2
    assert lib.frirl_hip_reducer_observe(None, None, None) == -2 and lib.frirl_hip_reducer_end_round(None) == -2
    assert lib.frirl_hip_reducer_result(None, None, C.byref(res)) == -2
    lib.frirl_hip_reducer_destroy(None)
