"""Host side of the per-agent exploration rows (no GPU needed): the new ABI symbols and the layout of struct frirl_hip_explore_rows,
the argument checks of the _explore entry points (those of their twins, in their order, EINVAL before ENODEV), the validation
frirl_hip_batch_set_exploration applies (frirl_hip_explore_rows_check: the same code without a batch), the rate
frirl_hip_explore_epsilon against the contract's formula bit for bit, and the --explore parsing of frirl_demo."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import explore_rows_cases as xc
from tests.test_external_host import _valid_call
from tests.test_hparam_rows_host import _learn_call, _message

NEW = ("frirl_hip_learn_run_explore", "frirl_hip_learn_train_explore", "frirl_hip_agent_begin_explore", "frirl_hip_agent_observe_explore",
       "frirl_hip_batch_set_exploration", "frirl_hip_explore_rows_check", "frirl_hip_explore_epsilon")


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    X = C.POINTER(frirl_amd.ExploreRowsDesc)
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    for twin in ("learn_run", "learn_train", "agent_begin", "agent_observe"):      # the _rows arguments with `explore` after `rows`
        a, x = frirl_amd.SIGNATURES[f"frirl_hip_{twin}_rows"][1], frirl_amd.SIGNATURES[f"frirl_hip_{twin}_explore"][1]
        assert x == a[:4] + [X] + a[4:], twin
    assert frirl_amd.SIGNATURES["frirl_hip_explore_epsilon"] == (C.c_double, [C.c_double, C.c_int32, C.c_uint32])
    assert frirl_amd.SIGNATURES["frirl_hip_explore_rows_check"][1] == [X, C.c_int32, C.POINTER(frirl_amd.AgentDesc)]
    assert frirl_amd.SIGNATURES["frirl_hip_batch_set_exploration"][1] == [C.c_void_p, X]
    for fn in (frirl_amd.agent_begin, frirl_amd.agent_observe, frirl_amd.train_persistent, frirl_amd.train):
        assert "explore" in inspect.signature(fn).parameters, fn.__name__
    assert list(inspect.signature(frirl_amd.ExploreRows.__init__).parameters) == ["self", "E", "device", "epsilon", "horizon", "horizon_all"]
    assert callable(frirl_amd.batch_set_exploration) and callable(frirl_amd.explore_epsilon)
    assert hasattr(frirl_amd.dropin(), "frirl_demo_parse_explore") and hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_explore")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(frirl_hip_explore_rows, f))
int main(void)
{
    printf("size %zu\n", sizeof(frirl_hip_explore_rows));
    F(epsilon); F(horizon); F(horizon_all); F(reserved);
    printf("agent %zu\nhparam_rows %zu\n", sizeof(frirl_hip_agent), sizeof(frirl_hip_hparam_rows));
    return 0;
}
"""


def test_struct_is_24_bytes_with_pinned_offsets(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert seen == dict(size=24, epsilon=0, horizon=8, horizon_all=16, reserved=20, agent=448, hparam_rows=48)
    R = frirl_amd.ExploreRowsDesc
    assert C.sizeof(R) == 24 and [(k, getattr(R, k).offset) for k, _ in R._fields_] == [("epsilon", 0), ("horizon", 8), ("horizon_all", 16), ("reserved", 20)]


def _forms(addr):
    """(rows, explore) pairs: both NULL, explore all NULL, explore with both columns, and each of those beside full hyper-parameter rows."""
    full_h = frirl_amd.HparamRowsDesc(*([addr] * 6))
    full_x = frirl_amd.ExploreRowsDesc(addr, addr, 3, 0)
    xs = [None, C.byref(frirl_amd.ExploreRowsDesc()), C.byref(full_x)]
    return [(r, x) for r in (None, C.byref(full_h)) for x in xs], (full_h, full_x)


def test_agent_explore_calls_refuse_what_their_twins_refuse(lib):
    """Same return code and the same message (but for the call's own name) as frirl_hip_agent_begin_taught / _observe_taught."""
    import torch

    def both(kind, t, b, ag, ev, io, teacher):
        twin, fn = getattr(lib, f"frirl_hip_agent_{kind}_taught"), getattr(lib, f"frirl_hip_agent_{kind}_explore")
        rc0 = twin(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
        m0 = _message(lib, f"frirl_hip_agent_{kind}_taught")
        forms, keep = _forms(b.rb)
        for rows, explore in forms:
            rc = fn(C.byref(t), C.byref(b), C.byref(ag), rows, explore, C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
            assert rc == rc0 and _message(lib, f"frirl_hip_agent_{kind}_explore") == m0, (kind, rc, rc0, lib.frirl_hip_last_error())
        return rc0

    for kind in ("begin", "observe"):
        for nant, A in ((1, 3), (9, 3), (4, 33), (4, 0)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            for teacher in (None, b.rb):
                assert both(kind, t, b, ag, ev, io, teacher) == -2
        keep, t, b, ag, ev, io = _valid_call(4, 5)
        assert both(kind, t, b, ag, ev, None, None) == -2
        keep, t, b, ag, ev, io = _valid_call(4, 5)
        io.action_out = None
        assert both(kind, t, b, ag, ev, io, None) == -2
        keep, t, b, ag, ev, io = _valid_call(4, 5)
        ev.done = None
        assert both(kind, t, b, ag, ev, io, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    io.reward = None
    assert both("observe", t, b, ag, ev, io, b.rb) == -2 and b"reward" in lib.frirl_hip_last_error()
    assert b"frirl_hip_agent_observe_explore" in lib.frirl_hip_last_error()
    if not torch.cuda.is_available():           # valid arguments: no CPU fallback, the device check answers both alike
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            for kind in ("begin", "observe"):
                assert both(kind, t, b, ag, ev, io, None) == -1 and b"no CPU fallback" in lib.frirl_hip_last_error()


def test_learn_explore_calls_refuse_what_their_twins_refuse(lib):
    """frirl_hip_learn_run_explore / _train_explore against frirl_hip_learn_run / _train: same code, same message but for the name,
    for every form of the two structs.  Without a GPU the refusals after the shape checks are ENODEV from both."""
    import torch
    gpu = torch.cuda.is_available()

    def run(form, t, b, ag, ev, cv, nlive=2, budget=10, max_episodes=5, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        a, c = (C.byref(ag) if ag is not None else None), (C.byref(cv) if cv is not None else None)
        if form is False:
            return lib.frirl_hip_learn_run(C.byref(t), C.byref(b), a, C.byref(ev), c, None, nlive, budget, max_episodes, None, None, w, ws_bytes, None)
        return lib.frirl_hip_learn_run_explore(C.byref(t), C.byref(b), a, form[0], form[1], C.byref(ev), c, None, nlive, budget, max_episodes, None, None, w, ws_bytes, None)

    def train(form, t, b, ag, ev, cv, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        no_cb = C.cast(None, frirl_amd.LEARN_CHUNK_FN)
        a, c = (C.byref(ag) if ag is not None else None), (C.byref(cv) if cv is not None else None)
        if form is False:
            return lib.frirl_hip_learn_train(C.byref(t), C.byref(b), a, C.byref(ev), c, 10, 5, None, None, None, w, ws_bytes, None, no_cb, None, None)
        return lib.frirl_hip_learn_train_explore(C.byref(t), C.byref(b), a, form[0], form[1], C.byref(ev), c, 10, 5, None, None, None, w, ws_bytes, None, no_cb, None, None)

    def same(call, name, *args, before_device=False, **kw):
        rc0 = call(False, *args, **kw)
        m0 = _message(lib, name)
        assert rc0 == (-2 if gpu or before_device else -1), (name, rc0, lib.frirl_hip_last_error())
        forms, keep = _forms(args[1].rb)
        for form in forms:
            rc = call(form, *args, **kw)
            assert rc == rc0 and _message(lib, name + "_explore") == m0, (name, rc, lib.frirl_hip_last_error(), m0)

    for c in (dict(), dict(nant=5, A=3, env_kind=2)):
        for call, name in ((run, "frirl_hip_learn_run"), (train, "frirl_hip_learn_train")):
            keep, t, b, ag, ev, cv = _learn_call(**c)
            same(call, name, t, b, None, ev, cv, before_device=True)              # NULL agent: EINVAL before ENODEV
            same(call, name, t, b, ag, ev, None)                                  # NULL convergence state
            keep, t, b, ag, ev, cv = _learn_call(**c)
            same(call, name, t, b, ag, ev, cv, ws=False)                          # no workspace
            same(call, name, t, b, ag, ev, cv, ws_bytes=64)                       # too small a workspace
            keep, t, b, ag, ev, cv = _learn_call(**c)
            ev.done = None
            same(call, name, t, b, ag, ev, cv, before_device=True)
        keep, t, b, ag, ev, cv = _learn_call(**c)
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, nlive=0)
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, budget=-1)
        keep, t, b, ag, ev, cv = _learn_call(**c)
        b.uidx = None
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv)                        # no index mirror
        keep, t, b, ag, ev, cv = _learn_call(**c)
        ag.p = 2
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv)                        # a shape frirl_hip_learn_supported does not cover


def _agent(eps=0.0):
    ag = frirl_amd.AgentDesc()
    ag.epsilon = eps
    return ag


def _check(lib, E, ag=None, epsilon=None, horizon=None, horizon_all=0, reserved=0):
    desc = frirl_amd.ExploreRowsDesc()
    desc.horizon_all, desc.reserved = horizon_all, reserved
    e = None if epsilon is None else np.ascontiguousarray(epsilon, dtype=np.float64)
    h = None if horizon is None else np.ascontiguousarray(horizon, dtype=np.int32)
    if e is not None:
        assert e.shape == (E,)
        desc.epsilon = e.ctypes.data
    if h is not None:
        assert h.shape == (E,)
        desc.horizon = h.ctypes.data
    ag = ag if ag is not None else _agent()
    return lib.frirl_hip_explore_rows_check(C.byref(desc), E, C.byref(ag)), lib.frirl_hip_last_error()


def test_rows_validation_names_agent_and_column(lib):
    """What frirl_hip_batch_set_exploration rejects before it copies anything (the same function, frirl_hip_explore_rows_check):
    an epsilon that is not finite or outside [0, 1], a horizon outside 0 .. 2^30, a horizon_all outside it, a reserved field that
    is not 0; the ends of the ranges pass."""
    E = 7
    assert _check(lib, E, epsilon=np.linspace(0.0, 1.0, E), horizon=[0, 1, 2, 3, 2 ** 30, 0, 7], horizon_all=2 ** 30)[0] == 0
    assert _check(lib, E)[0] == 0 and lib.frirl_hip_explore_rows_check(None, E, C.byref(_agent())) == 0
    for bad in (float("nan"), float("inf"), float("-inf"), -1e-300, 1.0000000000000002, 2.0):
        v = np.full(E, 0.3)
        v[4] = bad
        rc, msg = _check(lib, E, epsilon=v, horizon=np.zeros(E))
        assert rc == -2 and b"agent 4" in msg and b"epsilon" in msg, (bad, msg)
    for bad in (-1, 2 ** 30 + 1, -2 ** 31):
        h = np.full(E, 3, dtype=np.int64)
        h[2] = bad
        rc, msg = _check(lib, E, epsilon=np.full(E, 0.3), horizon=h)
        assert rc == -2 and b"agent 2" in msg and b"horizon" in msg and b"horizon_all" not in msg, (bad, msg)
        rc, msg = _check(lib, E, horizon_all=bad)
        assert rc == -2 and b"horizon_all" in msg, (bad, msg)
    rc, msg = _check(lib, E, reserved=1)
    assert rc == -2 and b"reserved" in msg
    rc, msg = _check(lib, E, ag=_agent(1.5), horizon=np.zeros(E))                  # no epsilon column: the agent's own value counts
    assert rc == -2 and b"epsilon" in msg
    assert _check(lib, E, ag=_agent(1.5), epsilon=np.full(E, 0.5))[0] == 0
    assert lib.frirl_hip_explore_rows_check(None, 0, C.byref(_agent())) == -2 and lib.frirl_hip_explore_rows_check(None, 3, None) == -2
    assert lib.frirl_hip_batch_set_exploration(None, None) == -2 and b"frirl_hip_batch_set_exploration" in lib.frirl_hip_last_error()


def test_explore_epsilon_is_the_formula_bit_for_bit(lib):
    """frirl_hip_explore_epsilon -- the host build of the inline function the kernels call -- against the contract's formula in
    Python's correctly rounded float64 (explore_rows_cases.epsilon_at): no horizon, the first and the last episode of a horizon,
    the episode after it, the largest horizon, epsilon 0 and 1, and 1000 random triples."""
    H = xc.HORIZON_MAX
    triples = [(0.3, 0, 1), (0.3, 0, 2 ** 32 - 1), (0.3, 4, 1), (0.3, 4, 4), (0.3, 4, 5), (0.1, 3, 2), (0.1, 3, 3), (0.7, 1, 1), (0.7, 1, 2),
               (0.3, H, 1), (0.3, H, 2), (0.3, H, H), (0.3, H, H + 1), (0.3, H, H - 1), (1.0, 7, 3), (1.0, 0, 9), (0.0, 7, 3), (0.0, 0, 1), (0.0, 7, 8)]
    rng = np.random.default_rng(26)
    for _ in range(1000):
        h = int(rng.choice([rng.integers(1, 12), rng.integers(1, 1000), rng.integers(1, H + 1)]))
        k = int(rng.choice([rng.integers(1, h + 1), rng.integers(1, h + 1), rng.integers(1, 2 * h + 2)]))
        triples.append((float(rng.uniform(0.0, 1.0)), h, k))
    inside = 0
    for eps, h, k in triples:
        got, want = frirl_amd.explore_epsilon(eps, h, k), xc.epsilon_at(eps, h, k)
        assert xc.bits(got) == xc.bits(want), (eps, h, k, got, want)
        inside += int(0 < h and k <= h)
    assert inside > 500
    assert frirl_amd.explore_epsilon(0.3, 4, 1) == 0.3 and frirl_amd.explore_epsilon(0.3, 4, 4) == 0.3 * 0.25 and frirl_amd.explore_epsilon(0.3, 4, 5) == 0.0
    assert frirl_amd.explore_epsilon(0.3, 5, 0) == 0.3          # key 0 (roll-outs, callers without an episode counter): outside every horizon


def _demo(args, cwd):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    return subprocess.run([demo, "--env", "mountaincar"] + args, cwd=cwd, capture_output=True, text=True)


def test_demo_refuses_malformed_explore_files_with_the_line_number(lib, tmp_path):
    """Parsing happens before any device is touched: exit code 2, the file and the line on stderr, nothing on stdout."""
    cases = {
        "# two pairs\n0.3 4\n\n0.3\n": ("line 4", "fewer"),
        "0.3 4\n0.3 4 1   # one too many\n": ("line 2", "more"),
        "0.3 4\nabc 4\n": ("line 2", "fewer"),                              # a bad number
        "1.5 4\n": ("line 1", "epsilon"),                                   # epsilon > 1
        "0 0\n-0.1 0\n": ("line 2", "epsilon"),
        "nan 2\n": ("line 1", "epsilon"),
        "0.3 -1\n": ("line 1", "horizon"),                                  # a negative horizon
        "0.3 2.5\n": ("line 1", "horizon"),
        "0.3 1073741825\n": ("line 1", "horizon"),
        "": (None, "no epsilon / horizon pair"),
        "# only a comment\n\n   \n": (None, "no epsilon / horizon pair"),
    }
    for i, (text, (line, why)) in enumerate(cases.items()):
        f = tmp_path / f"x{i}.txt"
        f.write_text(text)
        r = _demo(["--agents", "4", "--explore", str(f)], tmp_path)
        assert r.returncode == 2 and r.stdout == "" and "--explore" in r.stderr and why in r.stderr, (text, r.returncode, r.stderr)
        assert line is None or (line + ":") in r.stderr, (text, r.stderr)
    r = _demo(["--agents", "4", "--explore", str(tmp_path / "missing.txt")], tmp_path)
    assert r.returncode == 2 and "cannot open" in r.stderr and r.stdout == ""
    good = tmp_path / "good.txt"
    good.write_text("0.3 4\n")
    for args in (["--agents", "4", "--merge"], ["--agents", "4", "--evaluate", "2", "--teach-best", "1"], []):         # the last: without --agents
        r = _demo(args + ["--explore", str(good)], tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr and "--explore" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
    r = _demo(["--agents", "4", "--seed", "7"], tmp_path)
    assert r.returncode == 2 and "--seed" in r.stderr and r.stdout == ""
    r = _demo(["--agents", "4", "--explore", str(good), "--seed", "x7"], tmp_path)
    assert r.returncode == 2 and "--seed" in r.stderr and r.stdout == ""


def test_parse_explore_returns_the_pairs_in_file_order(lib, tmp_path):
    D = frirl_amd.dropin()
    f = tmp_path / "x.txt"
    f.write_text("# epsilon horizon\n0 0   # greedy\n\n0.1 2\n0.3 4\n1 1073741824\n")
    D.frirl_demo_parse_explore.restype = C.c_int
    D.frirl_demo_parse_explore.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_int)), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    eps, hor, n, err = C.POINTER(C.c_double)(), C.POINTER(C.c_int)(), C.c_int(0), C.create_string_buffer(256)
    assert D.frirl_demo_parse_explore(str(f).encode(), C.byref(eps), C.byref(hor), C.byref(n), err, 256) == 0 and n.value == 4
    assert [(eps[i], hor[i]) for i in range(4)] == [(0.0, 0), (0.1, 2), (0.3, 4), (1.0, 2 ** 30)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(eps, C.c_void_p))
    libc.free(C.cast(hor, C.c_void_p))
    bad = tmp_path / "bad.txt"
    bad.write_text("0.3 4\n0.3 -2\n")
    assert D.frirl_demo_parse_explore(str(bad).encode(), C.byref(eps), C.byref(hor), C.byref(n), err, 256) == -1
    assert err.value.startswith(b"line 2:") and b"horizon" in err.value and n.value == 0 and not eps and not hor
