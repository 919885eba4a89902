"""CPU-side checks of the caller-stepped reduction against a set of start states (frirl_hip_batch_reducer_create_starts,
csrc/policy_batch.hip): the ABI surface, argument validation before the device is looked for, and the one walk body of
csrc/reduce_walk.h in both row layouts -- compact (node * K + ki, frirl_hip_reduce_walk_starts_check) and caller-stepped
(node * n + start, frirl_hip_reduce_walk_starts_rows_check) -- against the model's walk (tests/reduce_starts_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from tests import reduce_starts_ref as ref
from tests.test_reduce_batch_host import demo_args
from tests.test_reduce_starts_host import probe as probe_compact


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_symbols_and_signatures(lib):
    S = frirl_amd.SIGNATURES
    P = C.POINTER
    want = {
        "frirl_hip_batch_reducer_create_starts": (C.c_void_p, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), C.c_void_p, C.c_void_p,
                                                               P(frirl_amd.ReduceStarts), C.c_int, C.c_double, C.c_int, C.c_void_p]),
        "frirl_hip_batch_reducer_result_starts": (C.c_int, [C.c_void_p, P(frirl_amd.ReduceStartResult)]),
        "frirl_hip_batch_reducer_starts": (C.c_int, [C.c_void_p]),
        "frirl_hip_reduce_walk_starts_rows_check": (C.c_int, [C.c_int, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), P(C.c_double), P(C.c_int32),
                                                              P(C.c_double), C.c_double, C.c_double, P(C.c_uint32)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.BatchReducer, "result_starts") and callable(frirl_amd.reduce_external_batch_starts)
    assert lib.frirl_hip_batch_reducer_starts(None) == 0
    assert lib.frirl_hip_batch_reducer_result_starts(None, None) == -2


def test_create_starts_checks_its_arguments_before_the_device(lib):
    """Every bad argument returns NULL with the reason in frirl_hip_last_error, with or without a GPU; good arguments -- start_states
    NULL among them: the caller places the rows -- reach the device check, which on a host without one says so (no CPU fallback)."""
    import torch
    buf, addr, t, b, ag = demo_args()

    def starts(n=4, drop=0, states=None, count=None):
        return frirl_amd.ReduceStarts(n, drop, states, count)

    def create(t=t, b=b, ag=ag, st=starts(), strategy=1, depth=4):
        h = lib.frirl_hip_batch_reducer_create_starts(C.byref(t), C.byref(b), C.byref(ag), None, None, C.byref(st) if st is not None else None, strategy,
                                                      0.0, depth, None)
        return h, lib.frirl_hip_last_error()

    def refused(what, **kw):
        h, err = create(**kw)
        assert not h and what in err, (kw, err)

    refused(b"NULL starts", st=None)
    for bad in (0, -1, 257, 1 << 20):
        refused(b"start states outside 1..256", st=starts(n=bad))
    refused(b"strategy 3", strategy=3)
    refused(b"depth 13", depth=13)
    _, _, t9, b9, ag9 = demo_args(nant=9)
    refused(b"nant", t=t9, b=b9, ag=ag9)
    _, _, _, _, ag33 = demo_args()
    ag33.A = 33
    refused(b"A=33", ag=ag33)
    big = frirl_amd.RuleBases(1 << 14, 8, addr, addr)                  # 2^14 agents x 256 starts x 4095 nodes
    refused(b"too many rows", b=big, st=starts(n=256), depth=12)
    just = frirl_amd.RuleBases(((2 ** 31 - 1) // 2) // (4 * 7) + 1, 8, addr, addr)      # the first E beyond INT32_MAX / 2 rows at n = 4, depth 3
    refused(b"too many rows", b=just, depth=3)
    if torch.cuda.is_available():
        return                                          # the good arguments below would be dereferenced on the device
    for kw in (dict(), dict(st=starts(n=1)), dict(st=starts(n=256, drop=1, count=addr)), dict(depth=0), dict(depth=12),
               dict(b=frirl_amd.RuleBases(just.E - 1, 8, addr, addr), depth=3)):
        refused(b"no CPU fallback", **kw)


def probe_rows(lib, d, n, used, steps, reward, steps_inc, prev, good_above, tol):
    """the walk over caller-stepped rows: steps / reward [nodes][n], steps_inc / prev [n]"""
    used = np.ascontiguousarray(used, dtype=np.int32)
    steps = np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
    reward = np.ascontiguousarray(reward, dtype=np.float64).reshape(-1)
    steps_inc = np.ascontiguousarray(steps_inc, dtype=np.int32)
    prev = np.array(prev, dtype=np.float64)
    bits = C.c_uint32(0xDEAD)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = lib.frirl_hip_reduce_walk_starts_rows_check(d, len(used), n, used.ctypes.data_as(ip), steps.ctypes.data_as(ip), reward.ctypes.data_as(dp),
                                                     steps_inc.ctypes.data_as(ip), prev.ctypes.data_as(dp), good_above, tol, C.byref(bits))
    assert rc == 0, lib.frirl_hip_last_error()
    return bits.value, list(prev)


@pytest.mark.parametrize("tol", [0.0, 1.0])
def test_strided_and_compact_walks_match_the_model(lib, tol):
    """Random outcomes, d 0..4, K 1..5 used starts among n = K .. K + 3 with holes in the used list.  The columns of the starts that are
    not used hold outcomes that would reject every node (and a poisoned prev_reward): they must never be read or written."""
    rng = np.random.default_rng(41)
    good = -50.0
    patterns, with_holes, blocked_late = set(), 0, 0
    for _ in range(800):
        d, K = int(rng.integers(0, 5)), int(rng.integers(1, 6))
        n = K + int(rng.integers(0, 4))
        used = np.sort(rng.choice(n, K, replace=False))
        with_holes += used[-1] != K - 1
        nodes = max((1 << d) - 1, 1)
        steps_inc = rng.integers(5, 40, K)
        prev0 = 100.0 + 10.0 * np.arange(K)
        steps = np.where(rng.random((nodes, K)) < 0.9, steps_inc[None, :], steps_inc[None, :] + 1).astype(np.int32)
        step = 0.5 * (tol if tol > 0 else 1.0)
        reward = prev0[None, :] + rng.choice([0, 0, 0, 0, 1, -1, 2, -2, 3], (nodes, K)) * step * (1.0 if tol > 0 else (rng.random((nodes, K)) < 0.1))
        reward[rng.random((nodes, K)) < 0.02] = good - 1.0
        want = ref.walk(d, K, steps.tolist(), reward.tolist(), steps_inc.tolist(), prev0.tolist(), good, tol)
        assert probe_compact(lib, d, K, steps, reward, steps_inc, prev0, good, tol) == want, (d, K)
        # the same outcomes scattered over n columns
        wide_steps = np.full((nodes, n), -3, dtype=np.int32)
        wide_reward = np.full((nodes, n), good - 7.0)
        wide_inc, wide_prev = np.full(n, -1, dtype=np.int32), np.full(n, -1e300)
        wide_steps[:, used], wide_reward[:, used], wide_inc[used], wide_prev[used] = steps, reward, steps_inc, prev0
        bits, prev = probe_rows(lib, d, n, used, wide_steps, wide_reward, wide_inc, wide_prev, good, tol)
        assert (bits, [prev[k] for k in used]) == want, (d, K, n, used)
        assert all(prev[k] == -1e300 for k in range(n) if k not in used)
        patterns.add((d, K, want[0]))
        if d and K > 1:
            ok = [ref.accept(steps[0][i], reward[0][i], steps_inc[i], prev0[i], good, tol) for i in range(K)]
            blocked_late += ok[0] and not all(ok)
    assert len(patterns) > 60 and with_holes > 200 and blocked_late > 20


def test_rows_walk_probe_refuses_bad_arguments(lib):
    b = C.c_uint32()
    i2, d2 = (C.c_int32 * 2)(0, 1), (C.c_double * 2)()
    f = lib.frirl_hip_reduce_walk_starts_rows_check
    good = (1, 2, 2, i2, i2, d2, i2, d2, 0.0, 0.0, C.byref(b))

    def swap(pos, v):
        return good[:pos] + (v,) + good[pos + 1:]

    for args in (swap(0, 13), swap(0, -1), swap(1, 0), swap(1, 3), swap(2, 0), swap(2, 257), swap(3, None), swap(4, None), swap(5, None), swap(6, None),
                 swap(7, None), swap(10, None), swap(3, (C.c_int32 * 2)(0, 2)), swap(3, (C.c_int32 * 2)(-1, 1))):
        assert f(*args) == -2, args[:3]
    assert f(*good) == 0
    assert f(0, 1, 2, i2, None, None, i2, d2, 0.0, 0.0, C.byref(b)) == 0 and b.value == 0      # nothing on trial
