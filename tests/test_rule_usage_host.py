"""CPU-side checks of the rule usage, the rule order and the map-validated reduction over several orders (frirl_hip_rule_usage,
frirl_hip_rule_order, frirl_hip_reduce_batch_map_orders, frirl_hip_batch_reduce_all_map_orders; csrc/rule_usage.hip, csrc/policy_map.hip,
csrc/batch.hip): the ABI surface, every documented FRIRL_HIP_EINVAL case refused before the device is looked for with the function's
name in frirl_hip_last_error, and the workspace size rules."""
import ctypes as C

import pytest

import frirl_amd
from tests.test_policy_map_host import map_args, no_gpu


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_symbols_and_signatures(lib):
    S = frirl_amd.SIGNATURES
    P = C.POINTER
    want = {
        "frirl_hip_rule_usage_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
        "frirl_hip_rule_usage": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), P(frirl_amd.MapPoints),
                                           P(frirl_amd.RuleUsageOut), C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_rule_order": (C.c_int, [P(frirl_amd.RuleBases), C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        "frirl_hip_reduce_batch_map_orders_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
        "frirl_hip_reduce_batch_map_orders": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), C.c_void_p, P(frirl_amd.MapPoints),
                                                        C.c_int32, C.c_void_p, P(C.c_int32), P(frirl_amd.ReduceOrdersResult), P(C.c_int32), C.c_void_p,
                                                        C.c_size_t, C.c_void_p]),
        "frirl_hip_batch_reduce_all_map_orders": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, P(C.c_double), C.c_int, C.c_int32,
                                                            P(frirl_amd.ReduceOrdersResult), P(C.c_int32), P(frirl_amd.ReduceMapTotals)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    for name in ("rule_usage", "rule_order", "reduce_batch_map_orders"):
        assert hasattr(frirl_amd.Problem, name)
    assert hasattr(frirl_amd, "batch_reduce_all_map_orders") and frirl_amd.REDUCE_MAX_ORDERS == 16


def test_struct_layouts():
    R, O = frirl_amd.ReduceOrdersResult, frirl_amd.RuleUsageOut
    assert C.sizeof(R) == 24 and R.rules_after.offset == 4 and R.points.offset == 8 and R.chosen.offset == 12 and R.tries.offset == 16
    assert C.sizeof(O) == 24 and O.peak.offset == 8 and O.best.offset == 16


def test_rule_usage_arguments_are_checked_before_the_device(lib):
    buf, addr, t, b, ag, mp = map_args()
    out = frirl_amd.RuleUsageOut(addr, None, None)
    need = lib.frirl_hip_rule_usage_workspace_bytes(3, 3, 5)
    assert need >= 3 * 5 * (2 * 8 + 8 + 4 + 4)
    ws = addr + 4096
    err = lib.frirl_hip_last_error

    def call(t=t, b=b, ag=ag, mp=mp, out=out, wsp=ws, nbytes=need):
        rc = lib.frirl_hip_rule_usage(C.byref(t) if t else None, C.byref(b) if b else None, C.byref(ag) if ag else None, C.byref(mp) if mp else None,
                                      C.byref(out) if out else None, wsp, nbytes, None)
        assert rc != -2 or b"frirl_hip_rule_usage" in err() or b"rulebases" in err() or b"tables" in err()
        return rc

    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(mp=None), dict(out=None), dict(out=frirl_amd.RuleUsageOut(None, addr, addr))):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    for kw in (dict(ag=None), dict(mp=None), dict(out=None)):
        assert call(**kw) == -2 and b"frirl_hip_rule_usage" in err(), kw
    ag_null = map_args()[4]
    ag_null.action_ve = None
    assert call(ag=ag_null) == -2 and b"NULL" in err()
    assert call(mp=frirl_amd.MapPoints(5, 0, None, None, None)) == -2 and b"NULL" in err()
    for n in (0, -1):
        assert call(mp=frirl_amd.MapPoints(n, 0, addr, None, None)) == -2 and b"n=" in err()
    _, _, _, b_big, _, _ = map_args(E=1 << 20)
    assert call(b=b_big, mp=frirl_amd.MapPoints(1 << 12, 0, addr, None, None), nbytes=1 << 62) == -2 and b"2^31" in err()
    for A in (0, 33, -1):
        assert call(ag=map_args(A=A)[4]) == -2 and b"A=" in err()
    for nant in (1, 9, 16):
        _, _, tn, bn, _, _ = map_args(nant=nant)
        assert call(t=tn, b=bn, nbytes=1 << 20) == -2 and b"nant" in err()
    assert call(wsp=None) == -2 and b"workspace" in err() and b"frirl_hip_rule_usage" in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()             # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()        # short
    assert call(nbytes=0) == -2
    if no_gpu():
        for nant in (2, 3, 5, 8):
            _, _, tn, bn, _, _ = map_args(nant=nant)
            assert call(t=tn, b=bn, nbytes=lib.frirl_hip_rule_usage_workspace_bytes(nant, 3, 5)) == -1, err()
            assert b"no CPU fallback" in err()


def test_rule_order_arguments_are_checked_before_the_device(lib):
    buf, addr, t, b, ag, mp = map_args()
    err = lib.frirl_hip_last_error

    def call(b=b, nant=3, keys=None, descending=0, order=addr):
        return lib.frirl_hip_rule_order(C.byref(b) if b else None, nant, keys, descending, None, order, None)

    for kw in (dict(b=None), dict(order=None), dict(b=frirl_amd.RuleBases(3, 8, None, addr)), dict(b=frirl_amd.RuleBases(3, 8, addr, None))):
        assert call(**kw) == -2 and b"NULL" in err() and b"frirl_hip_rule_order" in err(), kw
    for bad in (frirl_amd.RuleBases(0, 8, addr, addr), frirl_amd.RuleBases(3, 0, addr, addr), frirl_amd.RuleBases(-1, 8, addr, addr)):
        assert call(b=bad) == -2 and b"frirl_hip_rule_order" in err()
    for nant in (1, 9, 0):
        assert call(nant=nant) == -2 and b"nant" in err() and b"frirl_hip_rule_order" in err()
    for d in (2, -1):
        assert call(descending=d) == -2 and b"descending" in err() and b"frirl_hip_rule_order" in err()
    if no_gpu():
        assert call() == -1 and b"no CPU fallback" in err()
        assert call(keys=addr, descending=1) == -1


def test_reduce_batch_map_orders_arguments_are_checked_before_the_device(lib):
    buf, addr, t, b, ag, mp = map_args()
    res = (frirl_amd.ReduceOrdersResult * 3)()
    K = 4
    need = lib.frirl_hip_reduce_batch_map_orders_workspace_bytes(3, 3, 8, 5, K)
    assert need > 0
    ws = addr + 4096
    err = lib.frirl_hip_last_error
    who = b"frirl_hip_reduce_batch_map_orders"

    def call(t=t, b=b, ag=ag, mp=mp, K=K, orders=addr, results=res, wsp=ws, nbytes=need):
        return lib.frirl_hip_reduce_batch_map_orders(C.byref(t) if t else None, C.byref(b) if b else None, C.byref(ag) if ag else None, None,
                                                     C.byref(mp) if mp else None, K, orders, None, results, None, wsp, nbytes, None)

    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(mp=None), dict(results=None), dict(orders=None)):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    for kw in (dict(ag=None), dict(mp=None), dict(results=None), dict(orders=None)):
        assert call(**kw) == -2 and who in err(), kw
    ag_null = map_args()[4]
    ag_null.action_ve = None
    assert call(ag=ag_null) == -2 and b"NULL" in err()
    assert call(mp=frirl_amd.MapPoints(5, 0, None, None, None)) == -2 and b"NULL" in err()
    for k in (0, 17, -1):
        assert call(K=k, nbytes=1 << 20) == -2 and b"K=" in err() and who in err()
    for n in (0, -1):
        assert call(mp=frirl_amd.MapPoints(n, 0, addr, None, None)) == -2 and b"n=" in err()
    _, _, _, b_big, _, _ = map_args(E=1 << 16)
    assert call(b=b_big, mp=frirl_amd.MapPoints(1 << 12, 0, addr, None, None), K=16, nbytes=1 << 62) == -2 and b"2^31" in err()
    for A in (0, 33):
        assert call(ag=map_args(A=A)[4]) == -2 and b"A=" in err()
    for nant in (1, 9):
        _, _, tn, bn, _, _ = map_args(nant=nant)
        assert call(t=tn, b=bn, nbytes=1 << 20) == -2 and b"nant" in err()
    assert call(b=frirl_amd.RuleBases(0, 8, addr, addr)) == -2
    assert call(wsp=None) == -2 and b"workspace" in err() and who in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()
    assert call(nbytes=0) == -2
    if no_gpu():
        for k in (1, 16):
            assert call(K=k, nbytes=lib.frirl_hip_reduce_batch_map_orders_workspace_bytes(3, 3, 8, 5, k)) == -1, err()
            assert b"no CPU fallback" in err()


def test_batch_reduce_all_map_orders_arguments(lib):
    err = lib.frirl_hip_last_error
    who = b"frirl_hip_batch_reduce_all_map_orders"
    fake = C.c_void_p(16)                                                 # never dereferenced: every case below is refused first
    for order_set in (0, 16, -1, 32):
        assert lib.frirl_hip_batch_reduce_all_map_orders(fake, order_set, 1, None, 1, 0, None, None, None) == -2
        assert b"order_set" in err() and who in err()
    assert lib.frirl_hip_batch_reduce_all_map_orders(None, 1, 1, None, 1, 0, None, None, None) == -2 and b"NULL batch" in err() and who in err()
    for n in (0, 257):
        assert lib.frirl_hip_batch_reduce_all_map_orders(fake, 5, n, None, 1, 0, None, None, None) == -2 and b"n=" in err() and who in err()
    assert lib.frirl_hip_batch_reduce_all_map_orders(fake, 5, 2, None, 1, 0, None, None, None) == -2 and b"NULL start states" in err()
    for cap in (-1, 513):
        st = (C.c_double * 8)()
        assert lib.frirl_hip_batch_reduce_all_map_orders(fake, 15, 1, st, 1, cap, None, None, None) == -2 and b"cap=" in err() and who in err()
    # the existing entry point keeps refusing strategies outside 1..2
    assert lib.frirl_hip_batch_reduce_all_map(fake, 3, 1, None, 1, 0, None, None) == -2 and b"strategy" in err()


def test_workspace_bytes(lib):
    """each query: a multiple of 16, non-decreasing in every argument, 0 for a non-positive argument"""
    grid = {"nant": (2, 3, 5, 8), "E": (1, 2, 6, 64, 4096), "maxR": (2, 8, 120, 512, 2048), "n": (1, 2, 70, 257, 4096), "K": (1, 2, 4, 16)}

    def sweep(f, names):
        base = [grid[k][1] for k in names]
        for i, k in enumerate(names):
            last = 0
            for v in grid[k]:
                a = list(base)
                a[i] = v
                got = f(*a)
                assert got > 0 and got % 16 == 0 and got >= last, (names, a)
                last = got
            for v in (0, -1):
                a = list(base)
                a[i] = v
                assert f(*a) == 0, (names, a)

    sweep(lib.frirl_hip_rule_usage_workspace_bytes, ("nant", "E", "n"))
    sweep(lib.frirl_hip_reduce_batch_map_orders_workspace_bytes, ("nant", "E", "maxR", "n", "K"))
    # usage: the snapped points, S, a* and the hit per point; orders: private slot bytes and best0 per (agent, order) besides the shared arrays
    assert lib.frirl_hip_rule_usage_workspace_bytes(5, 6, 70) == 6 * 70 * 4 * 8 + 6 * 70 * 8 + 2 * 6 * 70 * 4
    assert lib.frirl_hip_reduce_batch_map_orders_workspace_bytes(5, 6, 512, 70, 4) >= 6 * 4 * 512 + 6 * 512 * 4 + 6 * 70 * 4 * 8 + 6 * 4 * 70 * 4 + 6 * 24
