"""CPU-side checks of the batched rule-base reduction (frirl_hip_reduce_batch, csrc/reduce_batch.hip): the ABI surface, argument
validation before the device is looked for, the workspace size and depth rules, and the tree walk the close-round kernel runs
(csrc/reduce_walk.h through the host-only probe frirl_hip_reduce_walk_check; ReducePlan::close_round, csrc/reduce_plan.h, runs the
same rw_walk on the host) against a Python restatement of the reference's walk (frirl_sequential_run.c:212,222)."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_symbols_and_signatures(lib):
    S = frirl_amd.SIGNATURES
    P = C.POINTER
    want = {
        "frirl_hip_reduce_batch_depth": (C.c_int, [C.c_int32, C.c_int32]),
        "frirl_hip_reduce_batch_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
        "frirl_hip_reduce_batch": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_double, C.c_int, P(C.c_int32), P(frirl_amd.ReduceResult), C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_reduce_walk_check": (C.c_int, [C.c_int, P(C.c_int32), P(C.c_double), C.c_int, C.c_double, C.c_double, C.c_double, P(C.c_uint32),
                                                  P(C.c_double)]),
        "frirl_hip_batch_reduce_all": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, P(frirl_amd.ReduceResult), P(C.c_int32)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.Problem, "reduce_batch")
    assert hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_reduce_all")


def demo_args(nant=3, env_kind=0, E=3, maxR=8):
    buf = (C.c_double * 8192)()
    addr = (C.addressof(buf) + 15) & ~15
    t = frirl_amd.Tables(nant, 41, addr, addr)
    b = frirl_amd.RuleBases(E, maxR, addr, addr)
    ag = frirl_amd.AgentDesc()
    ag.A, ag.env_kind, ag.max_steps, ag.grid_values, ag.action_ve = 3, env_kind, 10, addr, addr
    for k in range(nant):
        ag.grid_len[k] = 3
    return buf, addr, t, b, ag


def test_arguments_are_checked_before_the_device(lib):
    """Every bad argument is FRIRL_HIP_EINVAL (-2) with or without a GPU; good arguments reach the device check, which on a host without
    one answers FRIRL_HIP_ENODEV (-1): there is no CPU fallback."""
    import torch
    buf, addr, t, b, ag = demo_args()
    res = (frirl_amd.ReduceResult * 3)()
    need = lib.frirl_hip_reduce_batch_workspace_bytes(3, 3, 8, 4)
    assert need > 0
    ws = addr + 4096

    def call(t=t, b=b, ag=ag, strategy=1, depth=4, results=res, wsp=ws, nbytes=need):
        return lib.frirl_hip_reduce_batch(C.byref(t), C.byref(b), C.byref(ag), None, None, None, strategy, 0.0, depth, None, results, wsp, nbytes, None)

    for strategy in (0, 3, -1):
        assert call(strategy=strategy) == -2 and b"strategy" in lib.frirl_hip_last_error()
    for depth in (-1, 13, 100):
        assert call(depth=depth) == -2 and b"depth" in lib.frirl_hip_last_error()
    assert call(results=None) == -2 and b"NULL" in lib.frirl_hip_last_error()
    assert call(wsp=None) == -2 and b"workspace" in lib.frirl_hip_last_error()
    assert call(wsp=ws + 8) == -2 and b"workspace" in lib.frirl_hip_last_error()           # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in lib.frirl_hip_last_error()      # short
    assert call(nbytes=0) == -2
    # depth 0 resolves to frirl_hip_reduce_batch_depth(E, A): the workspace must hold that depth
    d0 = lib.frirl_hip_reduce_batch_depth(3, 3)
    assert call(depth=0, nbytes=lib.frirl_hip_reduce_batch_workspace_bytes(3, 3, 8, d0) - 16) == -2
    _, _, t5, b5, ag_wrong = demo_args(nant=5, env_kind=0)                                  # mountaincar has 3 antecedents
    assert call(t=t5, b=b5, ag=ag_wrong) == -2 and b"env_kind" in lib.frirl_hip_last_error()
    _, _, _, _, ag_ext = demo_args(env_kind=3)
    assert call(ag=ag_ext) == -2 and b"env_kind" in lib.frirl_hip_last_error()
    _, _, t4, b4, ag4 = demo_args(nant=4, env_kind=2)
    assert call(t=t4, b=b4, ag=ag4) == -2
    b0 = frirl_amd.RuleBases(0, 8, addr, addr)
    assert call(b=b0) == -2
    if torch.cuda.is_available():
        return                                          # the ENODEV path is exercised on CPU-only hosts
    big = lib.frirl_hip_reduce_batch_workspace_bytes(3, 3, 8, 0)
    for depth, nbytes in ((4, need), (0, big), (12, lib.frirl_hip_reduce_batch_workspace_bytes(3, 3, 8, 12))):
        assert call(depth=depth, nbytes=nbytes) == -1, lib.frirl_hip_last_error()
        assert b"no CPU fallback" in lib.frirl_hip_last_error()
    assert lib.frirl_hip_batch_reduce_all(None, 1, 0.0, 0, None, None) == -2


def test_workspace_bytes(lib):
    f = lib.frirl_hip_reduce_batch_workspace_bytes
    for nant in (3, 5):
        for depth in range(0, 13):
            last = 0
            for E in (1, 2, 6, 64, 100, 4096, 65536):
                v = f(nant, E, 512, depth)
                assert v > 0 and v % 16 == 0 and v >= last, (nant, depth, E)
                last = v
            last = 0
            for maxR in (2, 8, 120, 512, 2048):
                v = f(nant, 64, maxR, depth)
                assert v > 0 and v % 16 == 0 and v >= last, (nant, depth, maxR)
                last = v
        for E in (1, 6, 4096):
            sizes = [f(nant, E, 512, d) for d in range(1, 13)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
            # depth 0 holds whatever depth the rule selects, for any action count
            for A in (1, 3, 21):
                assert f(nant, E, 512, 0) >= f(nant, E, 512, lib.frirl_hip_reduce_batch_depth(E, A))
    assert f(3, 0, 8, 1) == 0 and f(3, 4, 0, 1) == 0 and f(3, 4, 8, 13) == 0 and f(3, 4, 8, -1) == 0


def test_depth_rule(lib):
    f = lib.frirl_hip_reduce_batch_depth
    for A in (1, 3, 4, 5, 21, 32):
        last = 12
        for E in (1, 2, 4, 6, 64, 1000, 4096, 65536, 1 << 20):
            d = f(E, A)
            assert 1 <= d <= 12 and d <= last, (E, A, d)
            last = d
        assert f(1 << 20, A) == 1, "more agents than the chip holds rows: no speculation"
        assert f(1, A) >= f(64, A) > f(65536, A)
    for E in (1, 64, 4096):
        assert f(E, 3) >= f(E, 21), "8 lanes per row hold fewer rows than 4"
    # without a device 256 CUs are assumed: 256 x 3 workgroups x 8 rows = 6144 rows for up to 4 actions, 256 x 1 x 4 = 1024 beyond
    import torch
    if not torch.cuda.is_available():
        assert [f(E, 3) for E in (1, 6, 7, 64, 4096)] == [10, 10, 9, 6, 1]
        assert [f(E, 21) for E in (1, 2, 64, 4096)] == [10, 9, 4, 1]


def walk_restated(d, steps, reward, steps_inc, prev_reward, good_above, tol):
    """The walk of a round's tree, restated independently of csrc/reduce_walk.h: the acceptance test of frirl_sequential_run.c:212
    along the outcomes that happened, prev_reward carried from accepted removal to accepted removal (:222)."""
    bits = 0
    for k in range(d):
        lane = (1 << k) - 1 + bits
        diff = prev_reward - reward[lane]
        if reward[lane] > good_above and steps[lane] == steps_inc and abs(diff) <= tol:
            bits |= 1 << k
            prev_reward = reward[lane]
    return bits, prev_reward


def probe(lib, d, steps, reward, steps_inc, prev_reward, good_above, tol):
    steps = np.ascontiguousarray(steps, dtype=np.int32)
    reward = np.ascontiguousarray(reward, dtype=np.float64)
    bits, prev = C.c_uint32(0xDEAD), C.c_double(-1.0)
    rc = lib.frirl_hip_reduce_walk_check(d, steps.ctypes.data_as(C.POINTER(C.c_int32)), reward.ctypes.data_as(C.POINTER(C.c_double)), steps_inc,
                                         prev_reward, good_above, tol, C.byref(bits), C.byref(prev))
    assert rc == 0, lib.frirl_hip_last_error()
    return bits.value, prev.value


@pytest.mark.parametrize("tol", [0.0, 2.5])
def test_walk_matches_restatement_on_every_outcome_pattern(lib, tol):
    """All 2^d outcome patterns for d <= 4, each with the three ways a node is rejected: the nodes ON the pattern's path get outcomes
    that produce it, every other node a random outcome, so a walk that reads a wrong node leaves the pattern."""
    steps_inc, prev0, good = 37, 100.0, 0.0
    rng = np.random.default_rng(17)
    n_checked = 0
    for d in range(0, 5):
        n = (1 << d) - 1
        for pattern in range(1 << d):
            for reject_kind in ("steps", "reward_bad", "reward_off"):
                steps = np.where(rng.random(max(n, 1)) < 0.5, steps_inc, steps_inc + 1).astype(np.int32)
                reward = np.full(max(n, 1), prev0, dtype=np.float64)
                bits = 0
                for k in range(d):
                    node = (1 << k) - 1 + bits
                    if (pattern >> k) & 1:
                        steps[node], reward[node] = steps_inc, prev0
                        bits |= 1 << k
                    elif reject_kind == "steps":
                        steps[node], reward[node] = steps_inc + 1, prev0
                    elif reject_kind == "reward_bad":
                        steps[node], reward[node] = steps_inc, good - 1.0
                    else:
                        steps[node], reward[node] = steps_inc, prev0 + tol + 0.5
                want = walk_restated(d, steps, reward, steps_inc, prev0, good, tol)
                assert want[0] == pattern, (d, pattern, reject_kind)
                assert probe(lib, d, steps, reward, steps_inc, prev0, good, tol) == want
                n_checked += 1
    assert n_checked == 3 * (1 + 2 + 4 + 8 + 16)


@pytest.mark.parametrize("tol", [0.0, 1.0])
def test_walk_carries_prev_reward(lib, tol):
    """An accepted node whose reward differs from prev_reward (within the tolerance) moves prev_reward: a later node is then judged
    against the NEW value -- accepted only because of the carry, or rejected only because of it.  Also random trees."""
    steps_inc, good = 12, -50.0
    if tol > 0:
        # node 0 accepted at 100.8 (|100 - 100.8| <= 1); node 2 (after an accept) at 101.6: within 1 of 100.8, not of 100
        steps = np.array([12, 12, 12], dtype=np.int32)
        reward = np.array([100.8, 55.0, 101.6])
        assert probe(lib, 2, steps, reward, steps_inc, 100.0, good, tol) == (3, 101.6) == walk_restated(2, steps, reward, steps_inc, 100.0, good, tol)
        # node 2 at 99.4: within 1 of the old 100, not of the carried 100.8
        reward = np.array([100.8, 55.0, 99.4])
        assert probe(lib, 2, steps, reward, steps_inc, 100.0, good, tol) == (1, 100.8) == walk_restated(2, steps, reward, steps_inc, 100.0, good, tol)
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(400):
        d = int(rng.integers(1, 13))
        n = (1 << d) - 1
        steps = np.where(rng.random(n) < 0.8, steps_inc, steps_inc + 1).astype(np.int32)
        reward = 100.0 + rng.integers(-2, 3, n) * 0.5 * (tol if tol > 0 else 1.0)
        reward[rng.random(n) < 0.05] = good - 1.0
        want = walk_restated(d, steps, reward, steps_inc, 100.0, good, tol)
        assert probe(lib, d, steps, reward, steps_inc, 100.0, good, tol) == want
        seen.add(want[1])
    assert len(seen) > 1 or tol == 0.0        # with no tolerance an accepted reward equals prev_reward: nothing to carry
    # d = 0: nothing on trial
    assert probe(lib, 0, np.zeros(1, np.int32), np.zeros(1), 5, 7.0, 0.0, 0.0) == (0, 7.0)
    b, p = C.c_uint32(), C.c_double()
    assert lib.frirl_hip_reduce_walk_check(13, None, None, 0, 0.0, 0.0, 0.0, C.byref(b), C.byref(p)) == -2
    assert lib.frirl_hip_reduce_walk_check(2, None, None, 0, 0.0, 0.0, 0.0, C.byref(b), C.byref(p)) == -2
