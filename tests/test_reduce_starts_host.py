"""CPU-side checks of the reduction against a set of start states (frirl_hip_reduce_batch_starts, csrc/reduce_starts.hip): the ABI
surface, the layout of the two structs against a compiled C probe, argument validation before the device is looked for, the workspace
size and depth rules, the walk over nodes x starts the close kernel runs (csrc/reduce_walk.h: rw_walk_starts, through the host-only probe
frirl_hip_reduce_walk_starts_check) against the model's walk (tests/reduce_starts_ref.py), and the usage errors of
`frirl_demo --reduce-starts`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import reduce_starts_ref as ref
from tests.test_reduce_batch_host import demo_args
from tests.test_reduce_batch_host import probe as probe_one


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_symbols_and_signatures(lib):
    S = frirl_amd.SIGNATURES
    P = C.POINTER
    want = {
        "frirl_hip_reduce_batch_starts_depth": (C.c_int, [C.c_int32] * 3),
        "frirl_hip_reduce_batch_starts_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
        "frirl_hip_reduce_batch_starts": (C.c_int, [P(frirl_amd.Tables), P(frirl_amd.RuleBases), P(frirl_amd.AgentDesc), C.c_void_p, P(frirl_amd.ReduceStarts),
                                                    C.c_void_p, C.c_int, C.c_double, C.c_int, P(C.c_int32), P(frirl_amd.ReduceResult),
                                                    P(frirl_amd.ReduceStartResult), C.c_void_p, C.c_size_t, C.c_void_p]),
        "frirl_hip_reduce_walk_starts_check": (C.c_int, [C.c_int, C.c_int, P(C.c_int32), P(C.c_double), P(C.c_int32), P(C.c_double), C.c_double,
                                                         C.c_double, P(C.c_uint32)]),
        "frirl_hip_batch_reduce_all_starts": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int32, P(C.c_double), C.c_int,
                                                        P(frirl_amd.ReduceResult), P(frirl_amd.ReduceStartResult), P(C.c_int32)]),
    }
    for name, (res, args) in want.items():
        assert S[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert hasattr(frirl_amd.Problem, "reduce_batch_starts") and frirl_amd.REDUCE_MAX_STARTS == 256
    assert hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_reduce_all_starts")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void)
{
    printf("max_starts %d\n", FRIRL_HIP_REDUCE_MAX_STARTS);
    printf("frirl_hip_reduce_starts %zu\n", sizeof(frirl_hip_reduce_starts));
    F(frirl_hip_reduce_starts, n); F(frirl_hip_reduce_starts, drop_bad_starts); F(frirl_hip_reduce_starts, start_states);
    F(frirl_hip_reduce_starts, start_count);
    printf("frirl_hip_reduce_start_result %zu\n", sizeof(frirl_hip_reduce_start_result));
    F(frirl_hip_reduce_start_result, used); F(frirl_hip_reduce_start_result, steps_incremental);
    F(frirl_hip_reduce_start_result, baseline_reward); F(frirl_hip_reduce_start_result, reward);
    return 0;
}
"""


def test_struct_layouts_match_a_compiled_c_probe(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen.pop("max_starts")) == frirl_amd.REDUCE_MAX_STARTS == 256
    for name, T in (("frirl_hip_reduce_starts", frirl_amd.ReduceStarts), ("frirl_hip_reduce_start_result", frirl_amd.ReduceStartResult)):
        assert int(seen.pop(name)) == C.sizeof(T), name
        for field, _ in T._fields_:
            assert int(seen.pop(f"{name}.{field}")) == getattr(T, field).offset, (name, field)
    assert not seen
    assert C.sizeof(frirl_amd.ReduceStartResult) == 24 and C.sizeof(frirl_amd.ReduceStarts) == 24


def test_arguments_are_checked_before_the_device(lib):
    """Every bad argument is FRIRL_HIP_EINVAL (-2) with or without a GPU; good arguments reach the device check, which on a host without
    one answers FRIRL_HIP_ENODEV (-1): there is no CPU fallback."""
    import torch
    buf, addr, t, b, ag = demo_args()
    res = (frirl_amd.ReduceResult * 3)()
    n = 4
    need = lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, 4, n)
    assert need > 0
    ws = addr + 4096

    def starts(n=n, drop=0, states=addr, count=None):
        return frirl_amd.ReduceStarts(n, drop, states, count)

    def call(t=t, b=b, ag=ag, st=starts(), strategy=1, depth=4, results=res, wsp=ws, nbytes=need):
        return lib.frirl_hip_reduce_batch_starts(C.byref(t), C.byref(b), C.byref(ag), None, C.byref(st) if st is not None else None, None, strategy, 0.0,
                                                 depth, None, results, None, wsp, nbytes, None)

    assert call(st=None) == -2 and b"NULL" in lib.frirl_hip_last_error()
    assert call(st=starts(states=None)) == -2 and b"NULL" in lib.frirl_hip_last_error()
    assert call(results=None) == -2 and b"NULL" in lib.frirl_hip_last_error()
    for bad in (0, -1, 257, 1 << 20):
        assert call(st=starts(n=bad), nbytes=1 << 30) == -2 and b"start states" in lib.frirl_hip_last_error(), bad
    for strategy in (0, 3, -1):
        assert call(strategy=strategy) == -2 and b"strategy" in lib.frirl_hip_last_error()
    for depth in (-1, 13, 100):
        assert call(depth=depth) == -2 and b"depth" in lib.frirl_hip_last_error()
    for A in (0, 33):
        _, _, _, _, ag_a = demo_args()
        ag_a.A = A
        assert call(ag=ag_a) == -2 and b"A=" in lib.frirl_hip_last_error()
    assert call(wsp=None) == -2 and b"workspace" in lib.frirl_hip_last_error()
    assert call(wsp=ws + 8) == -2 and b"workspace" in lib.frirl_hip_last_error()           # misaligned
    assert call(nbytes=need - 16) == -2 and b"workspace" in lib.frirl_hip_last_error()      # short
    assert call(nbytes=lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, 4, n - 1)) == -2      # sized for fewer starts
    assert call(nbytes=0) == -2
    # depth 0 resolves to frirl_hip_reduce_batch_starts_depth(E, A, n): the workspace must hold that depth
    d0 = lib.frirl_hip_reduce_batch_starts_depth(3, 3, n)
    assert call(depth=0, nbytes=lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, d0, n) - 16) == -2
    _, _, t5, b5, ag_wrong = demo_args(nant=5, env_kind=0)                                  # mountaincar has 3 antecedents
    assert call(t=t5, b=b5, ag=ag_wrong) == -2 and b"env_kind" in lib.frirl_hip_last_error()
    _, _, _, _, ag_ext = demo_args(env_kind=3)
    assert call(ag=ag_ext) == -2 and b"env_kind" in lib.frirl_hip_last_error()
    _, _, t4, b4, ag4 = demo_args(nant=4, env_kind=2)
    assert call(t=t4, b=b4, ag=ag4) == -2
    _, _, _, _, ag_grid = demo_args()
    ag_grid.grid_len[1] = 0
    assert call(ag=ag_grid) == -2 and b"grid" in lib.frirl_hip_last_error()
    b0 = frirl_amd.RuleBases(0, 8, addr, addr)
    assert call(b=b0) == -2
    assert lib.frirl_hip_batch_reduce_all_starts(None, 1, 0.0, 0, 2, None, 0, None, None, None) == -2
    if torch.cuda.is_available():
        return                                          # the ENODEV path is exercised on CPU-only hosts
    big = lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, 0, n)
    for depth, nbytes in ((4, need), (0, big), (12, lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, 12, n))):
        assert call(depth=depth, nbytes=nbytes) == -1, lib.frirl_hip_last_error()
        assert b"no CPU fallback" in lib.frirl_hip_last_error()
    for st in (starts(drop=1), starts(count=addr), starts(n=1), starts(n=256)):
        assert call(st=st, nbytes=lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, 4, st.n)) == -1, lib.frirl_hip_last_error()


def test_workspace_bytes(lib):
    f = lib.frirl_hip_reduce_batch_starts_workspace_bytes
    one = lib.frirl_hip_reduce_batch_workspace_bytes
    for nant in (3, 5):
        for depth in (0, 1, 3, 6, 10, 12):
            for n in (1, 2, 16, 256):
                last = 0
                for E in (1, 2, 6, 64, 100, 4096):
                    v = f(nant, E, 512, depth, n)
                    assert v > 0 and v % 16 == 0 and v >= last, (nant, depth, n, E)
                    last = v
                last = 0
                for maxR in (2, 8, 120, 512, 2048):
                    v = f(nant, 64, maxR, depth, n)
                    assert v > 0 and v % 16 == 0 and v >= last, (nant, depth, n, maxR)
                    last = v
            last = 0
            for n in (1, 2, 3, 4, 16, 100, 256):
                v = f(nant, 64, 512, depth, n)
                assert v > 0 and v % 16 == 0 and v >= last and v >= one(nant, 64, 512, depth), (nant, depth, n)
                last = v
        assert f(3, 64, 512, 4, 8) <= f(5, 64, 512, 4, 8)      # non-decreasing in nant
        for E, n in ((1, 1), (6, 4), (64, 16)):
            sizes = [f(nant, E, 512, d, n) for d in range(1, 13)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
            for A in (1, 3, 21):                        # depth 0 holds whatever depth the rule selects, for any action count
                assert f(nant, E, 512, 0, n) >= f(nant, E, 512, lib.frirl_hip_reduce_batch_starts_depth(E, A, n), n)
    for bad in ((3, 0, 8, 1, 1), (3, 4, 0, 1, 1), (3, 4, 8, 13, 1), (3, 4, 8, -1, 1), (3, 4, 8, 1, 0), (3, 4, 8, 1, 257), (3, 4, 8, 1, -2)):
        assert f(*bad) == 0, bad


def test_depth_rule(lib):
    """the largest d in 1..10 with E * n * (2^d - 1) <= the resident rows, at least 1; one start: the rule of frirl_hip_reduce_batch"""
    f = lib.frirl_hip_reduce_batch_starts_depth
    import torch
    rows = {3: 6144, 21: 1024}                          # without a device 256 CUs are assumed (tests/test_reduce_batch_host.py)
    for A in (1, 3, 4, 5, 21, 32):
        for E in (1, 2, 3, 6, 7, 64, 1000, 4096, 1 << 20):
            assert f(E, A, 1) == lib.frirl_hip_reduce_batch_depth(E, A)
            last = 10
            for n in (1, 2, 3, 4, 16, 100, 256):
                d = f(E, A, n)
                assert 1 <= d <= last, (E, A, n, d)
                last = d
                assert d == lib.frirl_hip_reduce_batch_depth(E * n, A), "E agents x n starts fill the chip like E * n agents"
                if not torch.cuda.is_available() and A in rows:
                    assert d == 1 or E * n * ((1 << d) - 1) <= rows[A], (E, A, n, d)
                    assert d == 10 or E * n * ((2 << d) - 1) > rows[A], (E, A, n, d)
    if not torch.cuda.is_available():
        assert [f(64, 3, n) for n in (1, 4, 16, 256)] == [6, 4, 2, 1]
        assert [f(64, 21, n) for n in (1, 4, 16)] == [4, 2, 1]


def probe(lib, d, K, steps, reward, steps_inc, prev, good_above, tol):
    steps = np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
    reward = np.ascontiguousarray(reward, dtype=np.float64).reshape(-1)
    steps_inc = np.ascontiguousarray(steps_inc, dtype=np.int32)
    prev = np.array(prev, dtype=np.float64)
    bits = C.c_uint32(0xDEAD)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = lib.frirl_hip_reduce_walk_starts_check(d, K, steps.ctypes.data_as(ip), reward.ctypes.data_as(dp), steps_inc.ctypes.data_as(ip),
                                                prev.ctypes.data_as(dp), good_above, tol, C.byref(bits))
    assert rc == 0, lib.frirl_hip_last_error()
    return bits.value, list(prev)


@pytest.mark.parametrize("tol", [0.0, 1.0])
def test_walk_over_nodes_and_starts_matches_the_model(lib, tol):
    """Random trees, d 0..6, K 1..5: rewards on a lattice of half the tolerance around each start's prev_reward, so differences land
    exactly AT the tolerance (accepted, <=) and one lattice step beyond it; single starts that reject a node all the others accept."""
    rng = np.random.default_rng(29)
    good = -50.0
    patterns, carried, blocked_by_one = set(), 0, 0
    for _ in range(600):
        d, K = int(rng.integers(0, 7)), int(rng.integers(1, 6))
        nodes = max((1 << d) - 1, 1)
        steps_inc = rng.integers(5, 40, K)
        prev0 = 100.0 + 10.0 * np.arange(K)
        steps = np.where(rng.random((nodes, K)) < 0.93, steps_inc[None, :], steps_inc[None, :] + 1).astype(np.int32)
        step = 0.5 * (tol if tol > 0 else 1.0)
        reward = prev0[None, :] + rng.choice([0, 0, 0, 0, 1, -1, 2, -2, 3], (nodes, K)) * step * (1.0 if tol > 0 else (rng.random((nodes, K)) < 0.1))
        reward[rng.random((nodes, K)) < 0.02] = good - 1.0
        want = ref.walk(d, K, steps.tolist(), reward.tolist(), steps_inc.tolist(), prev0.tolist(), good, tol)
        got = probe(lib, d, K, steps, reward, steps_inc, prev0, good, tol)
        assert got == want, (d, K)
        patterns.add((d, want[0]))
        carried += want[1] != prev0.tolist()
        if d and K > 1:
            ok = [ref.accept(steps[0][i], reward[0][i], steps_inc[i], prev0[i], good, tol) for i in range(K)]
            blocked_by_one += sum(ok) == K - 1
    assert len(patterns) > 40 and blocked_by_one > 10
    assert carried > 10 or tol == 0.0        # with no tolerance an accepted reward equals prev_reward: nothing to carry
    # exactly at the tolerance, and the next double beyond it
    if tol > 0:
        assert probe(lib, 1, 2, [[7, 7]], [[101.0, 49.0]], [7, 7], [100.0, 50.0], good, tol) == (1, [101.0, 49.0])
        assert probe(lib, 1, 2, [[7, 7]], [[101.0, np.nextafter(49.0, 0.0)]], [7, 7], [100.0, 50.0], good, tol) == (0, [100.0, 50.0])
        # the carry is per start: node 2 (after an accept) is judged against each start's NEW prev_reward
        steps = [[7, 7]] * 3
        assert probe(lib, 2, 2, steps, [[100.8, 50.0], [0.0, 0.0], [101.6, 50.9]], [7, 7], [100.0, 50.0], good, tol) == (3, [101.6, 50.9])
        assert probe(lib, 2, 2, steps, [[100.8, 50.0], [0.0, 0.0], [101.6, 51.1]], [7, 7], [100.0, 50.0], good, tol) == (1, [100.8, 50.0])


def test_walk_with_one_start_is_the_single_start_walk(lib):
    rng = np.random.default_rng(3)
    for tol in (0.0, 1.0):
        for _ in range(300):
            d = int(rng.integers(0, 13))
            nodes = max((1 << d) - 1, 1)
            steps = np.where(rng.random(nodes) < 0.8, 12, 13).astype(np.int32)
            reward = 100.0 + rng.integers(-2, 3, nodes) * 0.5 * (tol if tol > 0 else 1.0)
            reward[rng.random(nodes) < 0.05] = -51.0
            bits, prev = probe_one(lib, d, steps, reward, 12, 100.0, -50.0, tol)
            assert probe(lib, d, 1, steps, reward, [12], [100.0], -50.0, tol) == (bits, [prev])


def test_walk_probe_refuses_bad_arguments(lib):
    b = C.c_uint32()
    one_i, one_d = (C.c_int32 * 1)(), (C.c_double * 1)()
    f = lib.frirl_hip_reduce_walk_starts_check
    assert f(13, 1, one_i, one_d, one_i, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(-1, 1, one_i, one_d, one_i, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(1, 0, one_i, one_d, one_i, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(1, 257, one_i, one_d, one_i, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(2, 1, None, None, one_i, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(0, 1, None, None, None, one_d, 0.0, 0.0, C.byref(b)) == -2
    assert f(0, 1, None, None, one_i, None, 0.0, 0.0, C.byref(b)) == -2
    assert f(0, 1, None, None, one_i, one_d, 0.0, 0.0, None) == -2
    assert f(0, 1, None, None, one_i, one_d, 0.0, 0.0, C.byref(b)) == 0 and b.value == 0      # nothing on trial


def test_demo_refuses_bad_reduce_starts_arguments(lib):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    full = ["--agents", "2", "--reduce", "1", "--reduce-all"]
    for args in (full + ["--reduce-starts", "0"], full + ["--reduce-starts", "-2"], full + ["--reduce-starts", "257"],
                 full + ["--reduce-starts", "2", "--spread", "-1"], full + ["--reduce-starts", "2", "--spread", "nan"],
                 ["--agents", "2", "--reduce", "1", "--reduce-starts", "2"],              # without --reduce-all
                 ["--agents", "2", "--reduce-all", "--reduce-starts", "2"],               # without --reduce S
                 ["--agents", "2", "--reduce", "3", "--reduce-all", "--reduce-starts", "2"],
                 ["--reduce", "1", "--reduce-all", "--reduce-starts", "2"],               # without --agents
                 full + ["--merge", "--reduce-starts", "2"]):
        r = subprocess.run([demo, "--env", "mountaincar"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--reduce-starts" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
