"""CPU-side checks of the recorded roll-outs (frirl_hip_rollout_record, csrc/rollout_record.hip) and of frirl_hip_batch_teach: the ABI
surface, the layout of the two structs against a compiled C probe, argument validation before the device is looked for, the option,
and the usage errors of `frirl_demo --teach-best`.

Not reachable from here: "E * n * T overflowing int64" (with E * n <= INT32_MAX and an int32 T the product stays below 2^62; the check
is kept for the header's promise), and the errors of frirl_hip_batch_teach that need a batch (a batch needs a device): they are in
tests/test_hip_rollout_record.py."""
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
        "frirl_hip_rollout_record": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), P(frirl_amd.RolloutLogDesc), C.c_void_p]),
        "frirl_hip_batch_teach": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(C.c_double), C.c_int32, P(C.c_uint8), P(frirl_amd.TeachResult)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.Problem, "rollout_record") and hasattr(frirl_amd.RolloutLog, "demonstration") and callable(frirl_amd.batch_teach)
    assert hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_evaluate_teach")


FIELDS = {"frirl_hip_rollout_log": "RolloutLogDesc", "frirl_hip_teach_result": "TeachResult"}


def test_struct_layouts_match_a_compiled_c_probe(lib, tmp_path):
    lines = []
    for cname, pyname in FIELDS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in getattr(frirl_amd, pyname)._fields_]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "frirl_hip.h"\nint main(void)\n{\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, pyname in FIELDS.items():
        T = getattr(frirl_amd, pyname)
        assert int(seen.pop(cname)) == C.sizeof(T), cname
        for field, _ in T._fields_:
            assert int(seen.pop(f"{cname}.{field}")) == getattr(T, field).offset, (cname, field)
    assert not seen
    assert C.sizeof(frirl_amd.RolloutLogDesc) == 16 + 13 * 8 and C.sizeof(frirl_amd.TeachResult) == 32
    assert frirl_amd.TeachResult.records_replayed.offset == 24


LOG_ARRAYS = ("obs", "action", "reward", "success", "start", "length")


def test_arguments_are_checked_before_the_device(lib):
    """Every bad argument is FRIRL_HIP_EINVAL (-2) with or without a GPU; good arguments reach the device check, which on a host
    without one answers FRIRL_HIP_ENODEV (-1): there is no CPU fallback."""
    import torch
    buf, addr, t, b, ag = demo_args()

    def log(n=2, episodes=2, T=40, **null):
        lg = frirl_amd.RolloutLogDesc()
        lg.n, lg.episodes, lg.T = n, episodes, T
        for name in LOG_ARRAYS:
            setattr(lg, name, None if name in null else addr)
        return lg

    def call(t=t, b=b, ag=ag, lg=log()):
        ref = lambda x: C.byref(x) if x is not None else None
        return lib.frirl_hip_rollout_record(ref(t), ref(b), ref(ag), ref(lg), None)

    err = lib.frirl_hip_last_error
    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(lg=None)):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    for name in LOG_ARRAYS:
        assert call(lg=log(**{name: True})) == -2 and b"NULL" in err(), name
    for bad in (0, -1):
        assert call(lg=log(n=bad)) == -2 and b"n=" in err()
        assert call(lg=log(episodes=bad)) == -2 and b"episodes=" in err()
    for bad in (1, 0, -5):
        assert call(lg=log(T=bad)) == -2 and b"T=" in err()
    many = frirl_amd.RuleBases(1 << 20, 8, addr, addr)
    assert call(b=many, lg=log(n=1 << 12)) == -2 and b"INT32_MAX" in err()                           # E * n = 2^32
    for A in (0, 33):
        _, _, _, _, agA = demo_args()
        agA.A = A
        assert call(ag=agA) == -2 and b"A=" in err()
    _, _, t5, b5, ag_wrong = demo_args(nant=5, env_kind=0)                                           # mountaincar has 3 antecedents
    assert call(t=t5, b=b5, ag=ag_wrong) == -2 and b"env_kind" in err()
    _, _, _, _, ag_ext = demo_args(env_kind=3)
    assert call(ag=ag_ext) == -2 and b"env_kind" in err()
    _, _, t4, b4, ag4 = demo_args(nant=4, env_kind=2)                                                # nant other than 3 / 5
    assert call(t=t4, b=b4, ag=ag4) == -2
    for bad in (0, 65):
        _, _, _, _, agg = demo_args()
        agg.grid_len[1] = bad
        assert call(ag=agg) == -2 and b"grid_len" in err()
    # frirl_hip_batch_teach: the one case that needs no batch
    res = frirl_amd.TeachResult()
    assert lib.frirl_hip_batch_teach(None, 0, 1, None, 1, None, C.byref(res)) == -2 and b"NULL" in err()
    if torch.cuda.is_available():
        return                                          # the ENODEV path is exercised on CPU-only hosts
    for p in (0, 2, 7):                                 # any Shepard power is accepted
        _, _, _, _, agp = demo_args()
        agp.p = p
        assert call(ag=agp) == -1, err()
        assert b"no CPU fallback" in err()
    _, _, t5, b5, ag5 = demo_args(nant=5, env_kind=2)
    assert call(t=t5, b=b5, ag=ag5) == -1
    assert call(lg=log(T=2, n=1, episodes=1)) == -1     # the smallest log


def test_option_default_range_and_round_trip(lib):
    name = "rollout_record_slices"
    got = C.c_int(12345)
    assert lib.frirl_hip_get_option(name.encode(), C.byref(got)) == 0
    if "FRIRL_HIP_ROLLOUT_RECORD_SLICES" not in os.environ:
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


def test_demo_refuses_bad_teach_arguments(lib):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    base = [demo, "--env", "mountaincar", "--agents", "2"]
    for args in (["--evaluate", "2", "--teach-best", "0"], ["--evaluate", "2", "--teach-best", "-1"], ["--evaluate", "2", "--teach-best", "2", "--teach-passes", "0"],
                 ["--evaluate", "2", "--teach-best", "2", "--teach-passes", "1025"], ["--teach-best", "2"]):      # the last: without --evaluate
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--teach-best" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
