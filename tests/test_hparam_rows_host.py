"""Host side of the per-agent hyper-parameter rows (no GPU needed): the new ABI symbols and the layout of struct
frirl_hip_hparam_rows, the argument checks of the _rows entry points (those of their twins, in their order, EINVAL before ENODEV),
the validation frirl_hip_batch_set_hparams applies (frirl_hip_hparam_rows_check: the same code without a batch), and the --hparams
parsing of frirl_demo."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests.test_external_host import _valid_call

NEW = ("frirl_hip_learn_run_rows", "frirl_hip_learn_train_rows", "frirl_hip_agent_begin_rows", "frirl_hip_agent_observe_rows",
       "frirl_hip_batch_set_hparams", "frirl_hip_batch_agent_report", "frirl_hip_hparam_rows_check")


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    for twin in ("learn_run", "learn_train"):          # the twin's arguments with `rows` after `agent`
        a, r = frirl_amd.SIGNATURES[f"frirl_hip_{twin}"][1], frirl_amd.SIGNATURES[f"frirl_hip_{twin}_rows"][1]
        assert r == a[:3] + [C.POINTER(frirl_amd.HparamRowsDesc)] + a[3:]
    for twin in ("agent_begin", "agent_observe"):      # (t, b, agent, rows, envs, io, teacher, stream)
        a, r = frirl_amd.SIGNATURES[f"frirl_hip_{twin}_taught"][1], frirl_amd.SIGNATURES[f"frirl_hip_{twin}_rows"][1]
        assert r == a[:3] + [C.POINTER(frirl_amd.HparamRowsDesc)] + a[3:]
    for fn in (frirl_amd.agent_begin, frirl_amd.agent_observe, frirl_amd.train_persistent, frirl_amd.train):
        assert "rows" in inspect.signature(fn).parameters, fn.__name__
    assert callable(frirl_amd.batch_set_hparams) and callable(frirl_amd.batch_agent_report) and frirl_amd.HparamRows is not None
    assert hasattr(frirl_amd.dropin(), "frirl_demo_parse_hparams") and hasattr(frirl_amd.dropin(), "frirl_demo_batch_run_hparams")


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "frirl_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(frirl_hip_hparam_rows, f))
int main(void)
{
    printf("size %zu\n", sizeof(frirl_hip_hparam_rows));
    F(alpha); F(gamma); F(qdiff_pos_boundary); F(qdiff_neg_boundary); F(weight_significant); F(skip_rules);
    return 0;
}
"""


def test_struct_is_48_bytes_with_pinned_offsets(lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    want = dict(size=48, alpha=0, gamma=8, qdiff_pos_boundary=16, qdiff_neg_boundary=24, weight_significant=32, skip_rules=40)
    assert seen == want
    R = frirl_amd.HparamRowsDesc
    assert C.sizeof(R) == 48 and {k: getattr(R, k).offset for k in frirl_amd.HP_COLUMNS} == {k: v for k, v in want.items() if k != "size"}
    assert frirl_amd.HP_COLUMNS == tuple(k for k, _ in R._fields_)


def _rows(addr):
    """None, an all-NULL struct and a struct with every column given."""
    full = frirl_amd.HparamRowsDesc(*([addr] * 6))
    return [None, C.byref(frirl_amd.HparamRowsDesc()), C.byref(full)], full


def _message(lib, name):
    return lib.frirl_hip_last_error().replace(name.encode(), b"<call>")


def test_agent_rows_calls_refuse_what_their_twins_refuse(lib):
    """Same return code and the same message (but for the call's own name) as frirl_hip_agent_begin_taught / _observe_taught, with
    rows NULL, all columns NULL and all columns given: the shape checks, NULL io fields, then the device."""
    import torch

    def both(kind, t, b, ag, ev, io, teacher):
        twin, rows_fn = getattr(lib, f"frirl_hip_agent_{kind}_taught"), getattr(lib, f"frirl_hip_agent_{kind}_rows")
        rc0 = twin(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
        m0 = _message(lib, f"frirl_hip_agent_{kind}_taught")
        forms, keep = _rows(b.rb)
        for rows in forms:
            rc = rows_fn(C.byref(t), C.byref(b), C.byref(ag), rows, C.byref(ev), C.byref(io) if io is not None else None, teacher, None)
            assert rc == rc0 and _message(lib, f"frirl_hip_agent_{kind}_rows") == m0, (kind, rc, rc0, lib.frirl_hip_last_error())
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
        b.maxR = 9
        assert both(kind, t, b, ag, ev, io, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    io.reward = None
    assert both("observe", t, b, ag, ev, io, b.rb) == -2 and b"reward" in lib.frirl_hip_last_error()
    assert b"frirl_hip_agent_observe_rows" in lib.frirl_hip_last_error()
    if not torch.cuda.is_available():           # valid arguments: no CPU fallback, the device check answers both alike
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            for kind in ("begin", "observe"):
                assert both(kind, t, b, ag, ev, io, None) == -1 and b"no CPU fallback" in lib.frirl_hip_last_error()


def _learn_call(env_kind=0, nant=3, A=3, U=41):
    keep, t, b, ag, ev, io = _valid_call(nant, A)
    t.U, ag.env_kind, b.uidx = U, env_kind, b.rb
    cv = frirl_amd.ConvergenceDesc(*([b.rb] * 7))
    return keep, t, b, ag, ev, cv


def test_learn_rows_calls_refuse_what_their_twins_refuse(lib):
    """frirl_hip_learn_run_rows / _train_rows against frirl_hip_learn_run / _train: same code, same message but for the name, for
    rows NULL, all columns NULL and all columns given.  The twins look for a device at the end of their shape checks, before they
    look at the convergence state, the shape's support, the index mirror, nlive and the workspace: without a GPU those refusals are
    ENODEV from both, with one EINVAL from both."""
    import torch
    gpu = torch.cuda.is_available()
    def run(rows_form, t, b, ag, ev, cv, nlive=2, budget=10, max_episodes=5, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        if rows_form is False:
            return lib.frirl_hip_learn_run(C.byref(t), C.byref(b), C.byref(ag) if ag is not None else None, C.byref(ev), C.byref(cv) if cv is not None else None,
                                           None, nlive, budget, max_episodes, None, None, w, ws_bytes, None)
        return lib.frirl_hip_learn_run_rows(C.byref(t), C.byref(b), C.byref(ag) if ag is not None else None, rows_form, C.byref(ev),
                                            C.byref(cv) if cv is not None else None, None, nlive, budget, max_episodes, None, None, w, ws_bytes, None)

    def train(rows_form, t, b, ag, ev, cv, ws=True, ws_bytes=1 << 30):
        w = b.rb if ws else None
        no_cb = C.cast(None, frirl_amd.LEARN_CHUNK_FN)
        if rows_form is False:
            return lib.frirl_hip_learn_train(C.byref(t), C.byref(b), C.byref(ag) if ag is not None else None, C.byref(ev), C.byref(cv) if cv is not None else None,
                                             10, 5, None, None, None, w, ws_bytes, None, no_cb, None, None)
        return lib.frirl_hip_learn_train_rows(C.byref(t), C.byref(b), C.byref(ag) if ag is not None else None, rows_form, C.byref(ev),
                                              C.byref(cv) if cv is not None else None, 10, 5, None, None, None, w, ws_bytes, None, no_cb, None, None)

    def same(call, name, *args, before_device=False, **kw):
        rc0 = call(False, *args, **kw)
        m0 = _message(lib, name)
        assert rc0 == (-2 if gpu or before_device else -1), (name, rc0, lib.frirl_hip_last_error())
        forms, keep = _rows(args[1].rb)
        for rows in forms:
            rc = call(rows, *args, **kw)
            assert rc == rc0 and _message(lib, name + "_rows") == m0, (name, rc, lib.frirl_hip_last_error(), m0)

    cases = [dict(), dict(nant=5, A=3, env_kind=2)]
    for c in cases:
        for call, name in ((run, "frirl_hip_learn_run"), (train, "frirl_hip_learn_train")):
            keep, t, b, ag, ev, cv = _learn_call(**c)
            same(call, name, t, b, None, ev, cv, before_device=True)              # NULL agent
            same(call, name, t, b, ag, ev, None)                                  # NULL convergence state
            keep, t, b, ag, ev, cv = _learn_call(**c)
            same(call, name, t, b, ag, ev, cv, ws=False)                          # no workspace
            same(call, name, t, b, ag, ev, cv, ws_bytes=64)                       # too small a workspace
            keep, t, b, ag, ev, cv = _learn_call(**c)
            ev.done = None
            same(call, name, t, b, ag, ev, cv, before_device=True)
        keep, t, b, ag, ev, cv = _learn_call(**c)
        cv.prev_rconc = None
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv)
        keep, t, b, ag, ev, cv = _learn_call(**c)
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, nlive=0)
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, nlive=5)               # more than b->E
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, budget=-1)
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv, max_episodes=0)
        keep, t, b, ag, ev, cv = _learn_call(**c)
        b.uidx = None
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv)                        # no index mirror
        keep, t, b, ag, ev, cv = _learn_call(**c)
        ag.p = 2
        same(run, "frirl_hip_learn_run", t, b, ag, ev, cv)                        # a shape frirl_hip_learn_supported does not cover


def _agent(pos=20.0, neg=-250.0):
    ag = frirl_amd.AgentDesc()
    ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = pos, neg
    return ag


def _check(lib, E, ag=None, **columns):
    desc, keep = frirl_amd.HparamRowsDesc(), []
    for k, v in columns.items():
        a = np.ascontiguousarray(v, dtype=np.int32 if k == "skip_rules" else np.float64)
        assert a.shape == (E,)
        keep.append(a)
        setattr(desc, k, a.ctypes.data)
    ag = ag if ag is not None else _agent()
    return lib.frirl_hip_hparam_rows_check(C.byref(desc), E, C.byref(ag)), lib.frirl_hip_last_error()


def test_rows_validation_names_agent_and_column(lib):
    """What frirl_hip_batch_set_hparams rejects before it copies anything (the same function, frirl_hip_hparam_rows_check): a double
    that is not finite, qdiff_pos_boundary < qdiff_neg_boundary (also against the batch's own value where one column is missing), a
    negative weight_significant, skip_rules outside 0 / 1; bounds as large as +-1e30 pass."""
    E = 7
    ok = dict(alpha=np.full(E, 0.5), gamma=np.full(E, 0.9), qdiff_pos_boundary=np.full(E, 1e30), qdiff_neg_boundary=np.full(E, -1e30),
              weight_significant=np.zeros(E), skip_rules=np.arange(E) % 2)
    assert _check(lib, E, **ok)[0] == 0
    assert _check(lib, E)[0] == 0 and lib.frirl_hip_hparam_rows_check(None, E, C.byref(_agent())) == 0
    assert _check(lib, E, qdiff_pos_boundary=np.full(E, 3.0), qdiff_neg_boundary=np.full(E, 3.0))[0] == 0         # equal bounds
    for bad in (float("nan"), float("inf"), float("-inf")):
        for col in frirl_amd.HP_COLUMNS[:5]:
            v = np.array(ok[col], dtype=np.float64)
            v[4] = bad
            rc, msg = _check(lib, E, **dict(ok, **{col: v}))
            assert rc == -2 and b"agent 4" in msg and col.encode() in msg and b"finite" in msg, (col, bad, msg)
    rc, msg = _check(lib, E, alpha=[0.5, 0.5, float("nan"), 0.5, 0.5, 0.5, 0.5])
    assert rc == -2 and b"agent 2" in msg and b"alpha" in msg
    pos, neg = np.full(E, 5.0), np.full(E, -5.0)
    pos[5] = -6.0
    rc, msg = _check(lib, E, qdiff_pos_boundary=pos, qdiff_neg_boundary=neg)
    assert rc == -2 and b"agent 5" in msg and b"qdiff_pos_boundary" in msg and b"qdiff_neg_boundary" in msg
    rc, msg = _check(lib, E, qdiff_pos_boundary=pos)                           # -6 against the agent's own -250: fine
    assert rc == 0
    rc, msg = _check(lib, E, ag=_agent(neg=-1.0), qdiff_pos_boundary=pos)      # ... against -1: not
    assert rc == -2 and b"agent 5" in msg and b"qdiff_pos_boundary" in msg
    rc, msg = _check(lib, E, ag=_agent(pos=1.0), qdiff_neg_boundary=np.array([0.0, 0, 0, 2.0, 0, 0, 0]))
    assert rc == -2 and b"agent 3" in msg and b"qdiff_neg_boundary" in msg
    w = np.full(E, 0.05)
    w[6] = -1e-300
    rc, msg = _check(lib, E, weight_significant=w)
    assert rc == -2 and b"agent 6" in msg and b"weight_significant" in msg
    for bad in (2, -1):
        s = np.ones(E, dtype=np.int32)
        s[1] = bad
        rc, msg = _check(lib, E, skip_rules=s)
        assert rc == -2 and b"agent 1" in msg and b"skip_rules" in msg
    assert lib.frirl_hip_hparam_rows_check(None, 0, C.byref(_agent())) == -2 and lib.frirl_hip_hparam_rows_check(None, 3, None) == -2


def test_batch_calls_refuse_a_null_batch(lib):
    assert lib.frirl_hip_batch_set_hparams(None, None) == -2 and b"frirl_hip_batch_set_hparams" in lib.frirl_hip_last_error()
    assert lib.frirl_hip_batch_agent_report(None, None, None, None, None, None) == -2 and b"frirl_hip_batch_agent_report" in lib.frirl_hip_last_error()
    with pytest.raises(TypeError):
        frirl_amd.batch_set_hparams(None, epsilon=[0.1])


def _demo(args, cwd):
    demo = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
    return subprocess.run([demo, "--env", "mountaincar"] + args, cwd=cwd, capture_output=True, text=True)


GOOD = "0.5 1.0 20 -250 0.05 1\n"


def test_demo_refuses_malformed_hparams_files_with_the_line_number(lib, tmp_path):
    """Parsing happens before any device is touched: exit code 2, the file and the line on stderr, nothing on stdout."""
    cases = {
        "# two sets\n" + GOOD + "\n0.5 1.0 20 -250 0.05\n": ("line 4", "fewer"),                    # five values
        GOOD + GOOD + "0.5 1.0 20 -250 0.05 1 7   # one too many\n": ("line 3", "more"),
        GOOD + "0.5 abc 20 -250 0.05 1\n": ("line 2", "fewer"),
        "0.5 1.0 20 -250 0.05 2\n": ("line 1", "skip_rules"),
        GOOD + "# c\n0.5 1.0 -300 -250 0.05 1\n": ("line 3", "qdiff_pos"),
        "0.5 1.0 20 -250 -0.05 1\n": ("line 1", "weight_thr"),
        "nan 1.0 20 -250 0.05 1\n": ("line 1", "finite"),
        "0.5 1.0 inf -250 0.05 1\n": ("line 1", "finite"),
        "": (None, "no hyper-parameter set"),                                                        # empty file
        "# only a comment\n\n   \n": (None, "no hyper-parameter set"),
    }
    for i, (text, (line, why)) in enumerate(cases.items()):
        f = tmp_path / f"h{i}.txt"
        f.write_text(text)
        r = _demo(["--agents", "4", "--hparams", str(f)], tmp_path)
        assert r.returncode == 2 and r.stdout == "" and "--hparams" in r.stderr and why in r.stderr, (text, r.returncode, r.stderr)
        assert line is None or (line + ":") in r.stderr, (text, r.stderr)
    r = _demo(["--agents", "4", "--hparams", str(tmp_path / "missing.txt")], tmp_path)
    assert r.returncode == 2 and "cannot open" in r.stderr and r.stdout == ""


def test_demo_refuses_hparams_with_merge_or_teach_best(lib, tmp_path):
    f = tmp_path / "h.txt"
    f.write_text(GOOD)
    for args in (["--agents", "4", "--merge"], ["--agents", "4", "--evaluate", "2", "--teach-best", "1"], []):   # the last: without --agents
        r = _demo(args + ["--hparams", str(f)], tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr and "--hparams" in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)


def test_parse_hparams_returns_the_sets_in_file_order(lib, tmp_path):
    D = frirl_amd.dropin()
    f = tmp_path / "h.txt"
    f.write_text("# alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules\n0.5 1.0 20 -250 0.05 1   # the demo's own\n\n0.25 0.9 1e30 -1e30 0.002 0\n")
    D.frirl_demo_parse_hparams.restype = C.c_int
    D.frirl_demo_parse_hparams.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    sets, n, err = C.POINTER(C.c_double)(), C.c_int(0), C.create_string_buffer(256)
    assert D.frirl_demo_parse_hparams(str(f).encode(), C.byref(sets), C.byref(n), err, 256) == 0 and n.value == 2
    assert [sets[i] for i in range(12)] == [0.5, 1.0, 20.0, -250.0, 0.05, 1.0, 0.25, 0.9, 1e30, -1e30, 0.002, 0.0]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(sets, C.c_void_p))
