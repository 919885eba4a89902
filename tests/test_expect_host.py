"""Host side of per-agent expected SARSA (no GPU needed): the new ABI symbols and the layout of struct frirl_hip_expect_rows, the argument
checks of the _expect entry points (those of their _target twins, in their order, EINVAL before ENODEV), the validation
frirl_hip_batch_set_expected applies (frirl_hip_expect_rows_check: the same code without a batch), the batch calls' refusals without a
batch, and the --expected / --expected-rows parsing and refusals of frirl_demo."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests.test_external_host import _valid_call
from tests.test_hparam_rows_host import _learn_call

NEW = ("frirl_hip_learn_run_expect", "frirl_hip_learn_train_expect", "frirl_hip_agent_observe_expect", "frirl_hip_batch_set_expected",
       "frirl_hip_batch_get_expected", "frirl_hip_expect_rows_check")


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def _said(lib, name):
    """The last error with the call's own name at its start replaced: what two entry points of one family must agree on."""
    m = lib.frirl_hip_last_error().decode()
    return "CALL" + m[len(name):] if m.startswith(name + ":") else m


def test_new_symbols_exported(lib):
    X = C.POINTER(frirl_amd.ExpectRowsDesc)
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    assert not hasattr(lib, "frirl_hip_agent_begin_expect"), "begin performs no update: there is no _begin_expect"
    for twin in ("learn_run", "learn_train", "agent_observe"):                 # the _target arguments with `expect` after `target`
        a, x = frirl_amd.SIGNATURES[f"frirl_hip_{twin}_target"][1], frirl_amd.SIGNATURES[f"frirl_hip_{twin}_expect"][1]
        assert x == a[:6] + [X] + a[6:], twin
    assert frirl_amd.SIGNATURES["frirl_hip_expect_rows_check"][1] == [X, C.c_int32]
    for fn in (frirl_amd.agent_observe, frirl_amd.train_persistent):
        assert list(inspect.signature(fn).parameters)[-1] == "expect", fn.__name__
    assert "expect" not in inspect.signature(frirl_amd.agent_begin).parameters
    assert list(inspect.signature(frirl_amd.ExpectRows.__init__).parameters) == ["self", "E", "device", "expected", "expected_all"]
    assert list(inspect.signature(frirl_amd.batch_set_expected).parameters) == ["batch", "expected", "expected_all"]
    assert list(inspect.signature(frirl_amd.batch_get_expected).parameters) == ["batch"]
    assert frirl_amd.ExpectRows.null(5).desc is None
    assert hasattr(frirl_amd.dropin(), "frirl_demo_parse_expected") and hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_expected")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(frirl_hip_expect_rows, f))
int main(void)
{
    frirl_hip_expect_rows x = {0};
    x.reserved = ~x.reserved;
    printf("size %zu\n", sizeof(frirl_hip_expect_rows));
    F(expected); F(expected_all); F(reserved);
    printf("reserved_unsigned %d\ntarget_rows %zu\n", x.reserved > 0, sizeof(frirl_hip_target_rows));
    return 0;
}
"""


def test_struct_is_16_bytes_with_pinned_offsets(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert seen == dict(size=16, expected=0, expected_all=8, reserved=12, reserved_unsigned=1, target_rows=16)
    R = frirl_amd.ExpectRowsDesc
    assert C.sizeof(R) == 16 and [(k, getattr(R, k).offset) for k, _ in R._fields_] == [("expected", 0), ("expected_all", 8), ("reserved", 12)]
    assert dict(R._fields_)["reserved"] is C.c_uint32


def _forms(addr):
    """(rows, explore, target, expect, the suffix of the name the refusal carries): expect NULL (the _target entry point answers, which
    hands a NULL target on to _explore), all zero, expected_all 1, a column -- alone and beside the three other structs."""
    full_h = frirl_amd.HparamRowsDesc(*([addr] * 6))
    full_x = frirl_amd.ExploreRowsDesc(addr, addr, 3, 0)
    full_t = frirl_amd.TargetRowsDesc(addr, 0, 0)
    xs = [frirl_amd.ExpectRowsDesc(), frirl_amd.ExpectRowsDesc(None, 1, 0), frirl_amd.ExpectRowsDesc(addr, 0, 0)]
    forms = []
    for r, x, t in ((None, None, None), (C.byref(full_h), C.byref(full_x), C.byref(full_t)), (None, C.byref(full_x), None)):
        forms.append((r, x, t, None, "_target" if t is not None else "_explore"))
        forms += [(r, x, t, C.byref(e), "_expect") for e in xs]
    return forms, (full_h, full_x, full_t, xs)


def test_agent_observe_expect_refuses_what_its_twin_refuses(lib):
    """Same return code and the same message (but for the call's own name) as frirl_hip_agent_observe_taught: EINVAL for every bad
    argument before the device is asked for."""
    import torch

    def both(t, b, ag, ev, io, teacher):
        rc0 = lib.frirl_hip_agent_observe_taught(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
        m0 = _said(lib, "frirl_hip_agent_observe_taught")
        forms, keep = _forms(b.rb)
        for rows, explore, target, expect, suffix in forms:
            rc = lib.frirl_hip_agent_observe_expect(C.byref(t), C.byref(b), C.byref(ag), rows, explore, target, expect, C.byref(ev),
                                                    C.byref(io) if io is not None else None, teacher, None)
            assert rc == rc0 and _said(lib, "frirl_hip_agent_observe" + suffix) == m0, (rc, rc0, suffix, lib.frirl_hip_last_error())
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
    assert lib.frirl_hip_last_error().startswith(b"frirl_hip_agent_observe_expect:")
    if not torch.cuda.is_available():           # valid arguments: no CPU fallback, the device check answers both alike
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            assert both(t, b, ag, ev, io, None) == -1 and b"no CPU fallback" in lib.frirl_hip_last_error()


def test_learn_expect_calls_refuse_bad_arguments_before_the_device(lib):
    """frirl_hip_learn_run_expect / _train_expect against frirl_hip_learn_run / _train for the arguments that are refused before any
    device is asked for (a NULL agent, a NULL env array): FRIRL_HIP_EINVAL with or without a GPU, the same message but for the name at
    its start, for every form of the four structs.  Without a GPU every later refusal is ENODEV from both."""
    import torch
    gpu = torch.cuda.is_available()
    no_cb = C.cast(None, frirl_amd.LEARN_CHUNK_FN)

    def run(form, t, b, ag, ev, cv):
        a = C.byref(ag) if ag is not None else None
        if form is False:
            return lib.frirl_hip_learn_run(C.byref(t), C.byref(b), a, C.byref(ev), C.byref(cv), None, 2, 10, 5, None, None, b.rb, 1 << 30, None)
        return lib.frirl_hip_learn_run_expect(C.byref(t), C.byref(b), a, form[0], form[1], form[2], form[3], C.byref(ev), C.byref(cv), None, 2, 10, 5, None, None, b.rb,
                                              1 << 30, None)

    def train(form, t, b, ag, ev, cv):
        a = C.byref(ag) if ag is not None else None
        if form is False:
            return lib.frirl_hip_learn_train(C.byref(t), C.byref(b), a, C.byref(ev), C.byref(cv), 10, 5, None, None, None, b.rb, 1 << 30, None, no_cb, None, None)
        return lib.frirl_hip_learn_train_expect(C.byref(t), C.byref(b), a, form[0], form[1], form[2], form[3], C.byref(ev), C.byref(cv), 10, 5, None, None, None, b.rb,
                                                1 << 30, None, no_cb, None, None)

    def same(call, name, want, *args):
        rc0 = call(False, *args)
        m0 = _said(lib, name)
        assert rc0 == want, (name, rc0, lib.frirl_hip_last_error())
        forms, keep = _forms(args[1].rb)
        for form in forms:
            rc = call(form, *args)
            assert rc == rc0 and _said(lib, name + form[4]) == m0, (name, form[4], rc, lib.frirl_hip_last_error(), m0)

    for c in (dict(), dict(nant=5, A=3, env_kind=2)):
        for call, name in ((run, "frirl_hip_learn_run"), (train, "frirl_hip_learn_train")):
            keep, t, b, ag, ev, cv = _learn_call(**c)
            same(call, name, -2, t, b, None, ev, cv)                               # NULL agent: EINVAL before ENODEV
            keep, t, b, ag, ev, cv = _learn_call(**c)
            ev.done = None
            same(call, name, -2, t, b, ag, ev, cv)                                 # NULL env array: EINVAL before ENODEV
            if not gpu:
                keep, t, b, ag, ev, cv = _learn_call(**c)
                same(call, name, -1, t, b, ag, ev, cv)                             # valid so far: the device check answers


def _check(lib, E, expected=None, expected_all=0, reserved=0):
    desc = frirl_amd.ExpectRowsDesc()
    desc.expected_all, desc.reserved = expected_all, reserved
    t = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8)
    if t is not None:
        assert t.shape == (E,)
        desc.expected = t.ctypes.data
    return lib.frirl_hip_expect_rows_check(C.byref(desc), E), lib.frirl_hip_last_error()


def test_expect_validation_names_the_agent(lib):
    """What frirl_hip_batch_set_expected rejects before it copies anything (the same function, frirl_hip_expect_rows_check): a reserved
    field that is not 0, then expected_all other than 0 / 1, then the first agent whose byte is not 0 / 1, named; E < 1."""
    E = 7
    assert _check(lib, E, expected=[0, 1, 0, 1, 1, 0, 0], expected_all=1)[0] == 0
    assert _check(lib, E)[0] == 0 and _check(lib, E, expected_all=1)[0] == 0 and lib.frirl_hip_expect_rows_check(None, E) == 0
    for bad in (2, 3, 255):
        v = np.zeros(E, dtype=np.uint8)
        v[4] = bad
        rc, msg = _check(lib, E, expected=v)
        assert rc == -2 and msg == b"frirl_hip_expect_rows_check: agent 4: expected %d is neither 0 nor 1" % bad, (bad, msg)
    v = np.array([0, 1, 2, 0, 9, 0, 0], dtype=np.uint8)
    rc, msg = _check(lib, E, expected=v)
    assert rc == -2 and b"agent 2:" in msg, msg                                   # the first bad agent
    for bad in (-1, 2, 2 ** 31 - 1):
        rc, msg = _check(lib, E, expected_all=bad)
        assert rc == -2 and msg == b"frirl_hip_expect_rows_check: expected_all %d is neither 0 nor 1" % bad, (bad, msg)
    rc, msg = _check(lib, E, expected=v, expected_all=5, reserved=1)
    assert rc == -2 and msg == b"frirl_hip_expect_rows_check: reserved is 1, not 0", msg
    rc, msg = _check(lib, E, expected_all=1, reserved=2 ** 32 - 1)
    assert rc == -2 and b"reserved is 4294967295" in msg, msg
    rc, msg = _check(lib, E, expected=v, expected_all=5)
    assert rc == -2 and b"expected_all" in msg and b"agent" not in msg
    assert lib.frirl_hip_expect_rows_check(None, 0) == -2 and b"frirl_hip_expect_rows_check" in lib.frirl_hip_last_error()


def test_batch_calls_refuse_a_null_batch(lib):
    out = np.zeros(4, dtype=np.uint8)
    assert lib.frirl_hip_batch_set_expected(None, None, 1) == -2 and b"frirl_hip_batch_set_expected" in lib.frirl_hip_last_error()
    assert lib.frirl_hip_batch_set_expected(None, out.ctypes.data, 0) == -2
    assert lib.frirl_hip_batch_set_expected(None, None, 0) == -2
    assert lib.frirl_hip_batch_get_expected(None, out.ctypes.data) == -2 and b"frirl_hip_batch_get_expected" in lib.frirl_hip_last_error()


def _demo(args, cwd):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    return subprocess.run([demo, "--env", "mountaincar"] + args, cwd=cwd, capture_output=True, text=True)


def test_demo_refuses_malformed_expected_files_and_option_mixes(lib, tmp_path):
    """Parsing happens before any device is touched: exit code 2, the file and the line on stderr, nothing on stdout -- the wording of
    the --target-rows file.  --expected and --expected-rows are refused with --merge, --gpus and --teach-best, without --agents, with a
    TD target, and together."""
    cases = {
        "# two flags\n0\n\n\n1 1\n": ("line 5", "more"),
        "0\nabc\n": ("line 2", "fewer"),
        "2\n": ("line 1", "neither 0 nor 1"),
        "1\n0.5\n": ("line 2", "neither 0 nor 1"),
        "-1\n": ("line 1", "neither 0 nor 1"),
        "nan\n": ("line 1", "neither 0 nor 1"),
        "": (None, "holds no flag"),
        "# only a comment\n\n   \n": (None, "holds no flag"),
    }
    for i, (text, (line, why)) in enumerate(cases.items()):
        f = tmp_path / f"t{i}.txt"
        f.write_text(text)
        r = _demo(["--agents", "4", "--expected-rows", str(f)], tmp_path)
        assert r.returncode == 2 and r.stdout == "" and "--expected-rows" in r.stderr and why in r.stderr, (text, r.returncode, r.stderr)
        assert line is None or (line + ":") in r.stderr, (text, r.stderr)
    r = _demo(["--agents", "4", "--expected-rows", str(tmp_path / "missing.txt")], tmp_path)
    assert r.returncode == 2 and "cannot open" in r.stderr and r.stdout == ""
    good = tmp_path / "good.txt"
    good.write_text("0\n1\n")
    for opt in (["--expected"], ["--expected-rows", str(good)]):
        for args in (["--agents", "4", "--merge"], ["--agents", "4", "--gpus", "1"], ["--agents", "4", "--evaluate", "2", "--teach-best", "1"], [],
                     ["--agents", "4", "--target", "q"]):
            r = _demo(args + opt, tmp_path)
            assert r.returncode == 2 and "usage" in r.stderr and opt[0] in r.stderr and r.stdout == "", (args, opt, r.returncode, r.stderr)
    r = _demo(["--agents", "4", "--expected", "--expected-rows", str(good)], tmp_path)
    assert r.returncode == 2 and "exclude each other" in r.stderr and r.stdout == ""
    bad = tmp_path / "bad.txt"
    bad.write_text("0.3\n")                       # an --explore file with one value: its own wording and refusal
    r = _demo(["--agents", "4", "--expected", "--explore", str(bad)], tmp_path)
    assert r.returncode == 2 and "--explore" in r.stderr and "line 1:" in r.stderr and r.stdout == ""


def test_parse_expected_returns_the_column_in_file_order(lib, tmp_path):
    D = frirl_amd.dropin()
    f = tmp_path / "t.txt"
    f.write_text("# flags\n0   # sarsa\n\n1\n1\n0\n")
    D.frirl_demo_parse_expected.restype = C.c_int
    D.frirl_demo_parse_expected.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    col, n, err = C.POINTER(C.c_ubyte)(), C.c_int(0), C.create_string_buffer(256)
    assert D.frirl_demo_parse_expected(str(f).encode(), C.byref(col), C.byref(n), err, 256) == 0 and n.value == 4
    assert [col[i] for i in range(4)] == [0, 1, 1, 0]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(col, C.c_void_p))
    bad = tmp_path / "bad.txt"
    bad.write_text("1\n7\n")
    assert D.frirl_demo_parse_expected(str(bad).encode(), C.byref(col), C.byref(n), err, 256) == -1
    assert err.value.startswith(b"line 2:") and b"expected" in err.value and n.value == 0 and not col
