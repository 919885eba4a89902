"""CPU-side checks of the batched roll-outs (frirl_hip_rollout_batch, csrc/rollout_batch.hip): the ABI surface, the layout of the two
structs against a compiled C probe, argument validation before the device is looked for, the workspace-size rules, the three options,
and the usage errors of `frirl_demo --evaluate`."""
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
        "frirl_hip_rollout_batch_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
        "frirl_hip_rollout_batch": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), P(frirl_amd.RolloutBatchDesc),
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_batch_evaluate": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_double), P(frirl_amd.RolloutScore), P(C.c_int32)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.Problem, "rollout_batch") and callable(frirl_amd.rollout_scores)
    assert hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_evaluate")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void)
{
    printf("frirl_hip_rollout_batch_rows %zu\n", sizeof(frirl_hip_rollout_batch_rows));
    F(frirl_hip_rollout_batch_rows, n); F(frirl_hip_rollout_batch_rows, start_states); F(frirl_hip_rollout_batch_rows, row_count);
    F(frirl_hip_rollout_batch_rows, step_cap); F(frirl_hip_rollout_batch_rows, active); F(frirl_hip_rollout_batch_rows, steps);
    F(frirl_hip_rollout_batch_rows, reward); F(frirl_hip_rollout_batch_rows, success); F(frirl_hip_rollout_batch_rows, final_states);
    printf("frirl_hip_rollout_score %zu\n", sizeof(frirl_hip_rollout_score));
    F(frirl_hip_rollout_score, rows); F(frirl_hip_rollout_score, successes); F(frirl_hip_rollout_score, steps_sum);
    F(frirl_hip_rollout_score, reward_sum); F(frirl_hip_rollout_score, reward_min); F(frirl_hip_rollout_score, reward_max);
    return 0;
}
"""


def test_struct_layouts_match_a_compiled_c_probe(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, T in (("frirl_hip_rollout_batch_rows", frirl_amd.RolloutBatchDesc), ("frirl_hip_rollout_score", frirl_amd.RolloutScore)):
        assert int(seen.pop(name)) == C.sizeof(T), name
        for field, _ in T._fields_:
            assert int(seen.pop(f"{name}.{field}")) == getattr(T, field).offset, (name, field)
    assert not seen
    assert C.sizeof(frirl_amd.RolloutScore) == 40


def test_arguments_are_checked_before_the_device(lib):
    """Every bad argument is FRIRL_HIP_EINVAL (-2) with or without a GPU; good arguments reach the device check, which on a host
    without one answers FRIRL_HIP_ENODEV (-1): there is no CPU fallback."""
    import torch
    buf, addr, t, b, ag = demo_args()
    n = 4
    need = lib.frirl_hip_rollout_batch_workspace_bytes(3, 3, 8, n, 3)
    assert need > 0
    ws = addr + 4096

    def rows(n=n, steps=addr, reward=addr):
        return frirl_amd.RolloutBatchDesc(n, None, None, None, None, steps, reward, None, None)

    def call(t=t, b=b, ag=ag, ro=rows(), wsp=ws, nbytes=need, scores=None):
        ref = lambda x: C.byref(x) if x is not None else None
        return lib.frirl_hip_rollout_batch(ref(t), ref(b), ref(ag), ref(ro), scores, wsp, nbytes, None)

    err = lib.frirl_hip_last_error
    for kw in (dict(t=None), dict(b=None), dict(ag=None), dict(ro=None), dict(ro=rows(steps=None)), dict(ro=rows(reward=None))):
        assert call(**kw) == -2 and b"NULL" in err(), kw
    for bad_n in (0, -1):
        assert call(ro=rows(n=bad_n)) == -2 and b"n=" in err()
    many = frirl_amd.RuleBases(1 << 20, 8, addr, addr)
    assert call(b=many, ro=rows(n=1 << 12), nbytes=1 << 40) == -2 and b"INT32_MAX" in err()        # E * n = 2^32
    assert call(wsp=None) == -2 and b"workspace" in err()
    assert call(wsp=ws + 8) == -2 and b"workspace" in err()                                          # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in err()                                    # short
    assert call(nbytes=0) == -2
    _, _, t5, b5, ag_wrong = demo_args(nant=5, env_kind=0)                                           # mountaincar has 3 antecedents
    assert call(t=t5, b=b5, ag=ag_wrong) == -2 and b"env_kind" in err()
    _, _, _, _, ag_ext = demo_args(env_kind=3)
    assert call(ag=ag_ext) == -2 and b"env_kind" in err()
    _, _, t4, b4, ag4 = demo_args(nant=4, env_kind=2)                                                # nant other than 3 / 5
    assert call(t=t4, b=b4, ag=ag4) == -2
    for A in (0, 33):
        _, _, _, _, agA = demo_args()
        agA.A = A
        assert call(ag=agA) == -2 and b"A=" in err()
    assert lib.frirl_hip_batch_evaluate(None, 1, None, None, None) == -2
    if torch.cuda.is_available():
        return                                          # the ENODEV path is exercised on CPU-only hosts
    for p in (0, 2, 7):                                 # any Shepard power is accepted
        _, _, _, _, agp = demo_args()
        agp.p = p
        assert call(ag=agp) == -1, err()
        assert b"no CPU fallback" in err()
    _, _, t5, b5, ag5 = demo_args(nant=5, env_kind=2)
    assert call(t=t5, b=b5, ag=ag5, nbytes=lib.frirl_hip_rollout_batch_workspace_bytes(5, 3, 8, n, 3)) == -1


def test_workspace_bytes(lib):
    f = lib.frirl_hip_rollout_batch_workspace_bytes
    base = dict(nant=3, E=6, maxR=128, n=5, A=3)
    order = ("nant", "E", "maxR", "n", "A")
    sweeps = dict(nant=(3, 5), E=(1, 2, 6, 64, 4096, 65536), maxR=(2, 8, 120, 512, 2048), n=(1, 2, 5, 16, 70, 1024), A=(1, 3, 4, 5, 21, 32))
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
    assert f(3, 65536, 512, 16, 3) > f(3, 6, 512, 16, 3)


@pytest.mark.parametrize("name,default,values", [("rollout_batch_resident", -1, (0, 1, -1)), ("rollout_batch_resident_rules", 0, (120, 1, 0)),
                                                 ("rollout_batch_slices", 0, (1, 4, 16, 64, 0))])
def test_options_default_range_and_round_trip(lib, name, default, values):
    env = "FRIRL_HIP_" + name.upper()
    got = C.c_int(12345)
    assert lib.frirl_hip_get_option(name.encode(), C.byref(got)) == 0
    if env not in os.environ:
        assert got.value == default
    start = got.value
    try:
        for v in values:
            assert frirl_amd.set_option(name, v) in values + (start,)
            assert lib.frirl_hip_get_option(name.encode(), C.byref(got)) == 0 and got.value == v
    finally:
        frirl_amd.set_option(name, start)
    assert lib.frirl_hip_get_option((name + "_").encode(), C.byref(got)) == -2


def test_demo_refuses_bad_evaluate_arguments(lib):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    for args in (["--evaluate", "0"], ["--evaluate", "-3"], ["--evaluate", "4", "--spread", "-1"], ["--evaluate", "4", "--spread", "nan"],
                 ["--evaluate", "4"]):                                # the last: --evaluate without --agents
        r = subprocess.run([demo, "--env", "mountaincar"] + (["--agents", "2"] if args != ["--evaluate", "4"] else []) + args,
                           capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
