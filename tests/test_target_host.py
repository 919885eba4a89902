"""Host side of the per-agent TD target (no GPU needed): the new ABI symbols and the layout of struct frirl_hip_target_rows, the
argument checks of the _target entry points (those of their twins, in their order, EINVAL before ENODEV), the validation
frirl_hip_batch_set_target applies (frirl_hip_target_rows_check: the same code without a batch), the batch calls' refusals without a
batch, and the --target / --target-rows parsing and refusals of frirl_demo."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests.test_external_host import _valid_call
from tests.test_hparam_rows_host import _learn_call, _message

NEW = ("frirl_hip_learn_run_target", "frirl_hip_learn_train_target", "frirl_hip_agent_observe_target", "frirl_hip_batch_set_target",
       "frirl_hip_batch_get_target", "frirl_hip_target_rows_check")


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    T = C.POINTER(frirl_amd.TargetRowsDesc)
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    assert not hasattr(lib, "frirl_hip_agent_begin_target"), "begin performs no update: there is no _begin_target"
    for twin in ("learn_run", "learn_train", "agent_observe"):                 # the _explore arguments with `target` after `explore`
        a, x = frirl_amd.SIGNATURES[f"frirl_hip_{twin}_explore"][1], frirl_amd.SIGNATURES[f"frirl_hip_{twin}_target"][1]
        assert x == a[:5] + [T] + a[5:], twin
    assert frirl_amd.SIGNATURES["frirl_hip_target_rows_check"][1] == [T, C.c_int32]
    for fn in (frirl_amd.agent_observe, frirl_amd.train_persistent, frirl_amd.train):
        assert "target" in inspect.signature(fn).parameters, fn.__name__
    assert "target" not in inspect.signature(frirl_amd.agent_begin).parameters
    assert list(inspect.signature(frirl_amd.TargetRows.__init__).parameters) == ["self", "E", "device", "target", "target_all"]
    assert callable(frirl_amd.batch_set_target) and callable(frirl_amd.batch_get_target)
    assert (frirl_amd.TARGET_SARSA, frirl_amd.TARGET_Q) == (0, 1)
    assert hasattr(frirl_amd.dropin(), "frirl_demo_parse_target") and hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_target")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(frirl_hip_target_rows, f))
int main(void)
{
    printf("size %zu\n", sizeof(frirl_hip_target_rows));
    F(target); F(target_all); F(reserved);
    printf("sarsa %d\nq %d\nexplore_rows %zu\n", FRIRL_HIP_TARGET_SARSA, FRIRL_HIP_TARGET_Q, sizeof(frirl_hip_explore_rows));
    return 0;
}
"""


def test_struct_is_16_bytes_with_pinned_offsets(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert seen == dict(size=16, target=0, target_all=8, reserved=12, sarsa=0, q=1, explore_rows=24)
    R = frirl_amd.TargetRowsDesc
    assert C.sizeof(R) == 16 and [(k, getattr(R, k).offset) for k, _ in R._fields_] == [("target", 0), ("target_all", 8), ("reserved", 12)]


def _forms(addr):
    """(rows, explore, target, the name the refusal carries): target NULL (the _explore entry point answers), all zero, target_all Q, a
    column -- each alone and beside full hyper-parameter and exploration rows."""
    full_h = frirl_amd.HparamRowsDesc(*([addr] * 6))
    full_x = frirl_amd.ExploreRowsDesc(addr, addr, 3, 0)
    ts = [frirl_amd.TargetRowsDesc(), frirl_amd.TargetRowsDesc(None, 1, 0), frirl_amd.TargetRowsDesc(addr, 0, 0)]
    forms = []
    for r, x in ((None, None), (C.byref(full_h), C.byref(full_x)), (None, C.byref(full_x))):
        forms.append((r, x, None, "_explore"))
        forms += [(r, x, C.byref(t), "_target") for t in ts]
    return forms, (full_h, full_x, ts)


def test_agent_observe_target_refuses_what_its_twin_refuses(lib):
    """Same return code and the same message (but for the call's own name) as frirl_hip_agent_observe_taught."""
    import torch

    def both(t, b, ag, ev, io, teacher):
        rc0 = lib.frirl_hip_agent_observe_taught(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
        m0 = _message(lib, "frirl_hip_agent_observe_taught")
        forms, keep = _forms(b.rb)
        for rows, explore, target, suffix in forms:
            rc = lib.frirl_hip_agent_observe_target(C.byref(t), C.byref(b), C.byref(ag), rows, explore, target, C.byref(ev), C.byref(io) if io is not None else None,
                                                    teacher, None)
            assert rc == rc0 and _message(lib, "frirl_hip_agent_observe" + suffix) == m0, (rc, rc0, lib.frirl_hip_last_error())
        return rc0

    for nant, A in ((1, 3), (9, 3), (4, 33), (4, 0)):
        keep, t, b, ag, ev, io = _valid_call(nant, A)
        for teacher in (None, b.rb):
            assert both(t, b, ag, ev, io, teacher) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    assert both(t, b, ag, ev, None, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    io.action_out = None
    assert both(t, b, ag, ev, io, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    ev.done = None
    assert both(t, b, ag, ev, io, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    io.reward = None
    assert both(t, b, ag, ev, io, b.rb) == -2 and b"reward" in lib.frirl_hip_last_error()
    assert b"frirl_hip_agent_observe_target" in lib.frirl_hip_last_error()
    if not torch.cuda.is_available():           # valid arguments: no CPU fallback, the device check answers both alike
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            assert both(t, b, ag, ev, io, None) == -1 and b"no CPU fallback" in lib.frirl_hip_last_error()


def test_learn_target_calls_refuse_what_their_twins_refuse(lib):
    """frirl_hip_learn_run_target / _train_target against frirl_hip_learn_run / _train: same code, same message but for the name, for
    every form of the three structs.  Without a GPU the refusals after the shape checks are ENODEV from both."""
    import torch
    gpu = torch.cuda.is_available()

    def run(form, t, b, ag, ev, cv, nlive=2, budget=10, max_episodes=5, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        a, c = (C.byref(ag) if ag is not None else None), (C.byref(cv) if cv is not None else None)
        if form is False:
            return lib.frirl_hip_learn_run(C.byref(t), C.byref(b), a, C.byref(ev), c, None, nlive, budget, max_episodes, None, None, w, ws_bytes, None)
        return lib.frirl_hip_learn_run_target(C.byref(t), C.byref(b), a, form[0], form[1], form[2], C.byref(ev), c, None, nlive, budget, max_episodes, None, None, w,
                                              ws_bytes, None)

    def train(form, t, b, ag, ev, cv, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        no_cb = C.cast(None, frirl_amd.LEARN_CHUNK_FN)
        a, c = (C.byref(ag) if ag is not None else None), (C.byref(cv) if cv is not None else None)
        if form is False:
            return lib.frirl_hip_learn_train(C.byref(t), C.byref(b), a, C.byref(ev), c, 10, 5, None, None, None, w, ws_bytes, None, no_cb, None, None)
        return lib.frirl_hip_learn_train_target(C.byref(t), C.byref(b), a, form[0], form[1], form[2], C.byref(ev), c, 10, 5, None, None, None, w, ws_bytes, None, no_cb,
                                                None, None)

    def same(call, name, *args, before_device=False, **kw):
        rc0 = call(False, *args, **kw)
        m0 = _message(lib, name)
        assert rc0 == (-2 if gpu or before_device else -1), (name, rc0, lib.frirl_hip_last_error())
        forms, keep = _forms(args[1].rb)
        for form in forms:
            rc = call(form, *args, **kw)
            assert rc == rc0 and _message(lib, name + form[3]) == m0, (name, rc, lib.frirl_hip_last_error(), m0)

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


def _check(lib, E, target=None, target_all=0, reserved=0):
    desc = frirl_amd.TargetRowsDesc()
    desc.target_all, desc.reserved = target_all, reserved
    t = None if target is None else np.ascontiguousarray(target, dtype=np.uint8)
    if t is not None:
        assert t.shape == (E,)
        desc.target = t.ctypes.data
    return lib.frirl_hip_target_rows_check(C.byref(desc), E), lib.frirl_hip_last_error()


def test_target_validation_names_the_agent(lib):
    """What frirl_hip_batch_set_target rejects before it copies anything (the same function, frirl_hip_target_rows_check): a value
    other than 0 or 1 in the column or in target_all, a reserved field that is not 0, E < 1.  The order is that of
    frirl_hip_explore_rows_check: reserved, the _all field, then the agents in order."""
    E = 7
    assert _check(lib, E, target=[0, 1, 0, 1, 1, 0, 0], target_all=1)[0] == 0
    assert _check(lib, E)[0] == 0 and _check(lib, E, target_all=1)[0] == 0 and lib.frirl_hip_target_rows_check(None, E) == 0
    for bad in (2, 3, 255):
        v = np.zeros(E, dtype=np.uint8)
        v[4] = bad
        rc, msg = _check(lib, E, target=v)
        assert rc == -2 and b"agent 4" in msg and b"target" in msg and b"target_all" not in msg, (bad, msg)
    v = np.array([0, 1, 2, 0, 9, 0, 0], dtype=np.uint8)
    rc, msg = _check(lib, E, target=v)
    assert rc == -2 and b"agent 2" in msg, msg                                    # the first bad agent
    for bad in (-1, 2, 2 ** 31 - 1):
        rc, msg = _check(lib, E, target_all=bad)
        assert rc == -2 and b"target_all" in msg, (bad, msg)
    rc, msg = _check(lib, E, target=v, target_all=5, reserved=1)
    assert rc == -2 and b"reserved" in msg
    rc, msg = _check(lib, E, target=v, target_all=5)
    assert rc == -2 and b"target_all" in msg and b"agent" not in msg
    assert lib.frirl_hip_target_rows_check(None, 0) == -2 and b"frirl_hip_target_rows_check" in lib.frirl_hip_last_error()


def test_batch_calls_refuse_a_null_batch(lib):
    out = np.zeros(4, dtype=np.uint8)
    assert lib.frirl_hip_batch_set_target(None, None, 1) == -2 and b"frirl_hip_batch_set_target" in lib.frirl_hip_last_error()
    assert lib.frirl_hip_batch_set_target(None, out.ctypes.data, 0) == -2
    assert lib.frirl_hip_batch_get_target(None, out.ctypes.data) == -2 and b"frirl_hip_batch_get_target" in lib.frirl_hip_last_error()


def _demo(args, cwd):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    return subprocess.run([demo, "--env", "mountaincar"] + args, cwd=cwd, capture_output=True, text=True)


def test_demo_refuses_malformed_target_files_and_option_mixes(lib, tmp_path):
    """Parsing happens before any device is touched: exit code 2, the file and the line on stderr, nothing on stdout -- the wording of
    the --explore file.  --target and --target-rows are refused with --merge, --gpus and --teach-best, without --agents, and together."""
    cases = {
        "# two targets\n0\n\n\n1 1\n": ("line 5", "more"),
        "0\nabc\n": ("line 2", "fewer"),
        "2\n": ("line 1", "neither 0 (SARSA) nor 1 (Q)"),
        "1\n0.5\n": ("line 2", "neither 0 (SARSA) nor 1 (Q)"),
        "-1\n": ("line 1", "neither 0 (SARSA) nor 1 (Q)"),
        "nan\n": ("line 1", "neither 0 (SARSA) nor 1 (Q)"),
        "": (None, "holds no target"),
        "# only a comment\n\n   \n": (None, "holds no target"),
    }
    for i, (text, (line, why)) in enumerate(cases.items()):
        f = tmp_path / f"t{i}.txt"
        f.write_text(text)
        r = _demo(["--agents", "4", "--target-rows", str(f)], tmp_path)
        assert r.returncode == 2 and r.stdout == "" and "--target-rows" in r.stderr and why in r.stderr, (text, r.returncode, r.stderr)
        assert line is None or (line + ":") in r.stderr, (text, r.stderr)
    r = _demo(["--agents", "4", "--target-rows", str(tmp_path / "missing.txt")], tmp_path)
    assert r.returncode == 2 and "cannot open" in r.stderr and r.stdout == ""
    good = tmp_path / "good.txt"
    good.write_text("0\n1\n")
    for opt in (["--target", "q"], ["--target", "sarsa"], ["--target-rows", str(good)]):
        for args in (["--agents", "4", "--merge"], ["--agents", "4", "--gpus", "1"], ["--agents", "4", "--evaluate", "2", "--teach-best", "1"], []):
            r = _demo(args + opt, tmp_path)
            assert r.returncode == 2 and "usage" in r.stderr and opt[0] in r.stderr and r.stdout == "", (args, opt, r.returncode, r.stderr)
    r = _demo(["--agents", "4", "--target", "expected"], tmp_path)
    assert r.returncode == 2 and "--target needs sarsa or q" in r.stderr and r.stdout == ""
    r = _demo(["--agents", "4", "--target", "q", "--target-rows", str(good)], tmp_path)
    assert r.returncode == 2 and "exclude each other" in r.stderr and r.stdout == ""
    bad = tmp_path / "bad.txt"
    bad.write_text("0.3\n")                       # an --explore file with one value: its own wording and refusal
    r = _demo(["--agents", "4", "--target", "q", "--explore", str(bad)], tmp_path)
    assert r.returncode == 2 and "--explore" in r.stderr and "line 1:" in r.stderr and r.stdout == ""


def test_parse_target_returns_the_column_in_file_order(lib, tmp_path):
    D = frirl_amd.dropin()
    f = tmp_path / "t.txt"
    f.write_text("# target\n0   # sarsa\n\n1\n1\n0\n")
    D.frirl_demo_parse_target.restype = C.c_int
    D.frirl_demo_parse_target.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    col, n, err = C.POINTER(C.c_ubyte)(), C.c_int(0), C.create_string_buffer(256)
    assert D.frirl_demo_parse_target(str(f).encode(), C.byref(col), C.byref(n), err, 256) == 0 and n.value == 4
    assert [col[i] for i in range(4)] == [0, 1, 1, 0]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(col, C.c_void_p))
    bad = tmp_path / "bad.txt"
    bad.write_text("1\n7\n")
    assert D.frirl_demo_parse_target(str(bad).encode(), C.byref(col), C.byref(n), err, 256) == -1
    assert err.value.startswith(b"line 2:") and b"target" in err.value and n.value == 0 and not col
