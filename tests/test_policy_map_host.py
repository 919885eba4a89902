"""CPU-side checks of the policy map, the reduction validated on it and the points of recorded roll-outs (frirl_hip_policy_map,
frirl_hip_reduce_batch_map, frirl_hip_log_points; csrc/policy_map.hip): the ABI surface, every documented FRIRL_HIP_EINVAL case refused
before the device is looked for, and the workspace size rules."""
import ctypes as C

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
        "frirl_hip_policy_map_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
        "frirl_hip_policy_map": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), P(frirl_amd.MapPoints), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_reduce_batch_map_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
        "frirl_hip_reduce_batch_map": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), C.c_void_p, P(frirl_amd.MapPoints),
                                                 C.c_int, P(C.c_int32), P(frirl_amd.ReduceMapResult), C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_log_points_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
        "frirl_hip_log_points": (C.c_int, [P(frirl_amd.LogPointsDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    for name in ("policy_map", "reduce_batch_map"):
        assert hasattr(frirl_amd.Problem, name)
    assert hasattr(frirl_amd.RolloutLog, "points") and hasattr(frirl_amd, "grid_points") and hasattr(frirl_amd, "log_points")
    old = frirl_amd.set_option("reduce_map_resident", 0)
    assert old == -1 and frirl_amd.set_option("reduce_map_resident", old) == 0


def test_struct_layouts():
    M, R, L = frirl_amd.MapPoints, frirl_amd.ReduceMapResult, frirl_amd.LogPointsDesc
    assert C.sizeof(M) == 32 and M.points.offset == 8 and M.point_count.offset == 16 and M.active.offset == 24
    assert C.sizeof(R) == 16 and R.rules_after.offset == 4 and R.points.offset == 8 and R.tries.offset == 12
    assert C.sizeof(L) == 88 and L.cap.offset == 16 and L.only_successful.offset == 20 and L.obs.offset == 24 and L.success.offset == 40
    assert L.length.offset == 56 and L.points.offset == 64 and L.overflow.offset == 80


def map_args(nant=3, E=3, maxR=8, A=3, n=5):
    buf = (C.c_double * 8192)()
    addr = (C.addressof(buf) + 15) & ~15
    t = frirl_amd.Tables(nant, 41, addr, addr)
    b = frirl_amd.RuleBases(E, maxR, addr, addr)
    ag = frirl_amd.AgentDesc()
    ag.A, ag.env_kind, ag.action_ve = A, frirl_amd.ENV_EXTERNAL, addr          # env_kind is not read
    mp = frirl_amd.MapPoints(n, 0, addr, None, None)
    return buf, addr, t, b, ag, mp


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_policy_map_arguments_are_checked_before_the_device(lib):
    buf, addr, t, b, ag, mp = map_args()
    need = lib.frirl_hip_policy_map_workspace_bytes(3, 3, 5)
    assert need >= 3 * 5 * 2 * 8
    ws = addr + 4096
    err = lib.frirl_hip_last_error

    def call(t=t, b=b, ag=ag, mp=mp, best=addr, wsp=ws, nbytes=need):
        return lib.frirl_hip_policy_map(C.byref(t) if t else None, C.byref(b) if b else None, C.byref(ag) if ag else None,
                                        C.byref(mp) if mp else None, best, None, wsp, nbytes, None)

    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(mp=None), dict(best=None)):
        assert call(**kw) == -2 and b"NULL" in err(), kw
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
    assert call(wsp=None) == -2 and b"workspace" in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()             # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()        # short
    assert call(nbytes=0) == -2
    if no_gpu():
        for nant in (2, 3, 5, 8):
            _, _, tn, bn, _, _ = map_args(nant=nant)
            assert call(t=tn, b=bn, nbytes=lib.frirl_hip_policy_map_workspace_bytes(nant, 3, 5)) == -1, err()
            assert b"no CPU fallback" in err()


def test_reduce_batch_map_arguments_are_checked_before_the_device(lib):
    buf, addr, t, b, ag, mp = map_args()
    res = (frirl_amd.ReduceMapResult * 3)()
    need = lib.frirl_hip_reduce_batch_map_workspace_bytes(3, 3, 8, 5)
    assert need > 0
    ws = addr + 4096
    err = lib.frirl_hip_last_error

    def call(t=t, b=b, ag=ag, mp=mp, strategy=1, results=res, wsp=ws, nbytes=need):
        return lib.frirl_hip_reduce_batch_map(C.byref(t) if t else None, C.byref(b) if b else None, C.byref(ag) if ag else None, None,
                                              C.byref(mp) if mp else None, strategy, None, results, wsp, nbytes, None)

    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(mp=None), dict(results=None)):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    ag_null = map_args()[4]
    ag_null.action_ve = None
    assert call(ag=ag_null) == -2 and b"NULL" in err()
    assert call(mp=frirl_amd.MapPoints(5, 0, None, None, None)) == -2 and b"NULL" in err()
    for strategy in (0, 3, -1):
        assert call(strategy=strategy) == -2 and b"strategy" in err()
    for n in (0, -1):
        assert call(mp=frirl_amd.MapPoints(n, 0, addr, None, None)) == -2 and b"n=" in err()
    for A in (0, 33):
        assert call(ag=map_args(A=A)[4]) == -2 and b"A=" in err()
    for nant in (1, 9):
        _, _, tn, bn, _, _ = map_args(nant=nant)
        assert call(t=tn, b=bn, nbytes=1 << 20) == -2 and b"nant" in err()
    assert call(b=frirl_amd.RuleBases(0, 8, addr, addr)) == -2
    assert call(wsp=None) == -2 and b"workspace" in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()
    assert call(nbytes=0) == -2
    if no_gpu():
        for strategy in (1, 2):
            assert call(strategy=strategy) == -1, err()
            assert b"no CPU fallback" in err()


def test_log_points_arguments_are_checked_before_the_device(lib):
    buf = (C.c_double * 8192)()
    addr = (C.addressof(buf) + 15) & ~15
    need = lib.frirl_hip_log_points_workspace_bytes(2, 3, 12)
    assert need >= 2 * 3 * 12
    ws = addr + 32768
    err = lib.frirl_hip_last_error
    fields = [f for f, _ in frirl_amd.LogPointsDesc._fields_]

    def desc(**kw):
        v = dict(E=2, n_logs=3, T=12, ns=2, cap=40, only_successful=0, obs=addr, q_obs=addr, success=addr, start=addr, length=addr, points=addr,
                 point_count=addr, overflow=addr)
        v.update(kw)
        return frirl_amd.LogPointsDesc(*[v[f] for f in fields])

    def call(lp, wsp=ws, nbytes=need):
        return lib.frirl_hip_log_points(C.byref(lp) if lp else None, wsp, nbytes, None)

    assert call(None) == -2 and b"NULL" in err()
    for name in ("obs", "q_obs", "start", "length", "points", "point_count", "overflow"):
        assert call(desc(**{name: None})) == -2 and b"NULL" in err(), name
    assert call(desc(success=None, only_successful=1)) == -2 and b"NULL" in err()
    for name in ("E", "n_logs", "T", "cap"):
        for v in (0, -2):
            assert call(desc(**{name: v}), nbytes=1 << 20) == -2 and name.encode() in err(), name
    for ns in (0, 8):
        assert call(desc(ns=ns)) == -2 and b"ns=" in err()
    assert call(desc(E=1 << 12, n_logs=1 << 10, T=1 << 10), nbytes=1 << 62) == -2 and b"2^31" in err()
    assert call(desc(E=1 << 12, n_logs=1, T=1, cap=1 << 20), nbytes=1 << 62) == -2 and b"2^31" in err()
    assert call(desc(), wsp=None) == -2 and b"workspace" in err()
    assert call(desc(), wsp=ws + 8) == -2 and b"workspace" in err()
    assert call(desc(), nbytes=need - 16) == -2 and b"workspace" in err()
    assert call(desc(), nbytes=0) == -2
    if no_gpu():
        assert call(desc()) == -1 and b"no CPU fallback" in err()
        assert call(desc(success=None)) == -1, "success is optional without only_successful"


def test_workspace_bytes(lib):
    """each query: a multiple of 16, non-decreasing in every argument, 0 for a non-positive argument"""
    grid = {"nant": (2, 3, 5, 8), "E": (1, 2, 6, 64, 4096), "maxR": (2, 8, 120, 512, 2048), "n": (1, 2, 70, 257, 4096),
            "n_logs": (1, 3, 16), "T": (1, 12, 1001)}

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

    sweep(lib.frirl_hip_policy_map_workspace_bytes, ("nant", "E", "n"))
    sweep(lib.frirl_hip_reduce_batch_map_workspace_bytes, ("nant", "E", "maxR", "n"))
    sweep(lib.frirl_hip_log_points_workspace_bytes, ("E", "n_logs", "T"))
    # the map's workspace holds the snapped points; the reduction's also the order / alive / slot tables, best0 and the results
    assert lib.frirl_hip_policy_map_workspace_bytes(5, 6, 70) == 6 * 70 * 4 * 8
    assert lib.frirl_hip_reduce_batch_map_workspace_bytes(5, 6, 512, 70) >= 6 * 70 * 4 * 8 + 6 * 70 * 4 + 6 * 512 * 9 + 6 * 16
