"""CPU-side checks of the point-keeping roll-outs (frirl_hip_rollout_points, csrc/rollout_points.hip) and of
frirl_hip_batch_reduce_all_map: the ABI surface, the layout of the two structs against a compiled C probe, argument validation before
the device is looked for, the workspace-size rules, the option, and the usage errors of `frirl_demo --reduce-map`.

Not reachable from here: the errors of frirl_hip_batch_reduce_all_map that need a batch (a batch needs a device); they are in
tests/test_hip_rollout_points.py."""
import ctypes as C
import os
import subprocess

import pytest

import frirl_amd
from tests.test_reduce_batch_host import demo_args


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_symbols_and_signatures(lib):
    S = frirl_amd.SIGNATURES
    P = C.POINTER
    want = {
        "frirl_hip_rollout_points_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
        "frirl_hip_rollout_points": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), P(frirl_amd.RolloutPointsDesc),
                                               C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_batch_reduce_all_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, P(C.c_double), C.c_int, C.c_int32, P(frirl_amd.ReduceMapResult),
                                                     P(frirl_amd.ReduceMapTotals)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.Problem, "rollout_points") and callable(frirl_amd.batch_reduce_all_map) and frirl_amd.POINTS_MAX_CAP == 512
    assert hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_reduce_all_map")


FIELDS = {"frirl_hip_rollout_points_desc": "RolloutPointsDesc", "frirl_hip_reduce_map_totals": "ReduceMapTotals"}


def test_struct_layouts_match_a_compiled_c_probe(lib, tmp_path):
    lines = ['printf("cap %d\\n", FRIRL_HIP_POINTS_MAX_CAP);']
    for cname, pyname in FIELDS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in getattr(frirl_amd, pyname)._fields_]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "frirl_hip.h"\nint main(void)\n{\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen.pop("cap")) == frirl_amd.POINTS_MAX_CAP
    for cname, pyname in FIELDS.items():
        T = getattr(frirl_amd, pyname)
        assert int(seen.pop(cname)) == C.sizeof(T), cname
        for field, _ in T._fields_:
            assert int(seen.pop(f"{cname}.{field}")) == getattr(T, field).offset, (cname, field)
    assert not seen
    assert C.sizeof(frirl_amd.RolloutPointsDesc) == 16 + 9 * 8 and C.sizeof(frirl_amd.ReduceMapTotals) == 40
    assert frirl_amd.ReduceMapTotals.rules_before.offset == 16


OUT_ARRAYS = ("points", "point_count", "overflow")


def test_arguments_are_checked_before_the_device(lib):
    """Every bad argument is FRIRL_HIP_EINVAL (-2) with or without a GPU; good arguments reach the device check, which on a host
    without one answers FRIRL_HIP_ENODEV (-1): there is no CPU fallback."""
    import torch
    buf, addr, t, b, ag = demo_args()
    n, cap = 4, 16
    need = lib.frirl_hip_rollout_points_workspace_bytes(3, 3, 8, n, cap, 3)
    assert need > 0
    ws = addr + 4096

    def desc(n=n, cap=cap, only_successful=0, **null):
        rp = frirl_amd.RolloutPointsDesc()
        rp.n, rp.cap, rp.only_successful = n, cap, only_successful
        for name in OUT_ARRAYS:
            setattr(rp, name, None if name in null else addr)
        return rp

    def call(t=t, b=b, ag=ag, rp=desc(), wsp=ws, nbytes=need):
        ref = lambda x: C.byref(x) if x is not None else None
        return lib.frirl_hip_rollout_points(ref(t), ref(b), ref(ag), ref(rp), wsp, nbytes, None)

    err = lib.frirl_hip_last_error
    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(rp=None)):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    for name in OUT_ARRAYS:
        assert call(rp=desc(**{name: True})) == -2 and b"NULL" in err(), name
    for bad in (0, -1, 257):
        assert call(rp=desc(n=bad), nbytes=1 << 40) == -2 and b"n=" in err(), bad
    for bad in (0, -1, 513):
        assert call(rp=desc(cap=bad), nbytes=1 << 40) == -2 and b"cap=" in err(), bad
    for bad in (2, -1):
        assert call(rp=desc(only_successful=bad)) == -2 and b"only_successful" in err(), bad
    many = frirl_amd.RuleBases(1 << 24, 8, addr, addr)
    assert call(b=many, rp=desc(n=256), nbytes=1 << 60) == -2 and b"INT32_MAX" in err()              # E * n = 2^32
    assert call(b=many, rp=desc(n=1, cap=512), nbytes=1 << 60) == -2 and b"INT32_MAX" in err()       # E * cap = 2^33
    assert call(wsp=None) == -2 and b"workspace" in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()                                          # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()                                    # short
    assert call(nbytes=0) == -2
    _, _, t5, b5, ag_wrong = demo_args(nant=5, env_kind=0)                                           # mountaincar has 3 antecedents
    assert call(t=t5, b=b5, ag=ag_wrong, nbytes=1 << 40) == -2 and b"env_kind" in err()
    _, _, _, _, ag_ext = demo_args(env_kind=3)
    assert call(ag=ag_ext) == -2 and b"env_kind" in err()
    _, _, t4, b4, ag4 = demo_args(nant=4, env_kind=2)                                                # nant other than 3 / 5
    assert call(t=t4, b=b4, ag=ag4, nbytes=1 << 40) == -2
    for A in (0, 33):
        _, _, _, _, agA = demo_args()
        agA.A = A
        assert call(ag=agA) == -2 and b"A=" in err()
    for bad in (0, 65):
        _, _, _, _, agg = demo_args()
        agg.grid_len[1] = bad
        assert call(ag=agg) == -2 and b"grid_len" in err()
    # frirl_hip_batch_reduce_all_map: the one case that needs no batch
    tot = frirl_amd.ReduceMapTotals()
    assert lib.frirl_hip_batch_reduce_all_map(None, 1, 1, None, 1, 0, None, C.byref(tot)) == -2 and b"NULL" in err()
    if torch.cuda.is_available():
        return                                          # the ENODEV path is exercised on CPU-only hosts
    for p in (0, 2, 7):                                 # any Shepard power is accepted
        _, _, _, _, agp = demo_args()
        agp.p = p
        assert call(ag=agp) == -1, err()
        assert b"no CPU fallback" in err()
    _, _, t5, b5, ag5 = demo_args(nant=5, env_kind=2)
    assert call(t=t5, b=b5, ag=ag5, nbytes=lib.frirl_hip_rollout_points_workspace_bytes(5, 3, 8, n, cap, 3)) == -1
    assert call(rp=desc(n=1, cap=1, only_successful=1)) == -1                                        # the smallest call
    assert call(rp=desc(n=256, cap=512), nbytes=lib.frirl_hip_rollout_points_workspace_bytes(3, 3, 8, 256, 512, 3)) == -1      # the largest


def test_workspace_bytes(lib):
    f = lib.frirl_hip_rollout_points_workspace_bytes
    base = dict(nant=3, E=6, maxR=128, n=5, cap=64, A=3)
    order = ("nant", "E", "maxR", "n", "cap", "A")
    sweeps = dict(nant=(3, 5), E=(1, 2, 6, 64, 4096, 65536), maxR=(2, 8, 120, 512, 2048), n=(1, 2, 4, 5, 16, 70, 256), cap=(1, 8, 64, 511, 512),
                  A=(1, 3, 4, 5, 21, 32))
    for name, values in sweeps.items():
        last = 0
        for v in values:
            args = dict(base, **{name: v})
            got = f(*(args[k] for k in order))
            assert got > 0 and got % 16 == 0 and got >= last, (name, v, got, last)
            last = got
        for v in (0, -1):
            args = dict(base, **{name: v})
            assert f(*(args[k] for k in order)) == 0, (name, v)
    assert f(3, 65536, 512, 16, 512, 3) > f(3, 6, 512, 16, 512, 3)
    # the points of 65 536 agents with 16 starts: far below the 51 GB of records the log path would write
    assert f(3, 65536, 512, 16, 512, 3) < 4 << 30 and f(5, 65536, 512, 16, 512, 3) < 8 << 30


def test_option_default_range_and_round_trip(lib):
    name = "rollout_points_slices"
    got = C.c_int(12345)
    assert lib.frirl_hip_get_option(name.encode(), C.byref(got)) == 0
    if "FRIRL_HIP_ROLLOUT_POINTS_SLICES" not in os.environ:
        assert got.value == 0
    start = got.value
    values = (1, 4, 8, 16, 0)
    try:
        for v in values:
            assert frirl_amd.set_option(name, v) in values + (start,)
            assert lib.frirl_hip_get_option(name.encode(), C.byref(got)) == 0 and got.value == v
    finally:
        frirl_amd.set_option(name, start)
    assert lib.frirl_hip_get_option((name + "_").encode(), C.byref(got)) == -2


def test_demo_refuses_bad_reduce_map_arguments(lib):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    base = [demo, "--env", "mountaincar", "--agents", "2"]
    full = ["--reduce", "1", "--reduce-all"]
    for args in (full + ["--reduce-map", "0"], full + ["--reduce-map", "-1"], full + ["--reduce-map", "257"],
                 full + ["--reduce-map", "4", "--reduce-starts", "4"],                 # the two exclude each other
                 full + ["--reduce-starts", "4", "--reduce-map", "4"],
                 full + ["--reduce-map", "4", "--spread", "-1"],
                 ["--reduce", "1", "--reduce-map", "4"],                                 # without --reduce-all
                 ["--reduce-all", "--reduce-map", "4"],                                  # without --reduce
                 ["--reduce", "3", "--reduce-all", "--reduce-map", "4"],                 # a strategy that does not exist
                 full + ["--reduce-map", "4", "--merge"],
                 full + ["--reduce-map-all"]):                                          # without --reduce-map
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--reduce-map K" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
    r = subprocess.run([demo, "--env", "mountaincar"] + full + ["--reduce-map", "4"], capture_output=True, text=True)      # without --agents
    assert r.returncode == 2 and "usage" in r.stderr and r.stdout == ""
