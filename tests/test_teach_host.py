"""Host side of imitation (no GPU needed): the new ABI symbols, the layout of struct frirl_hip_demonstration, and the argument checks
of frirl_hip_agent_begin_taught / _observe_taught and frirl_hip_learn_demonstration (EINVAL before ENODEV, no CPU fallback)."""
import ctypes as C

import pytest

import frirl_amd
from tests.test_external_host import _valid_call


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    for n in ("frirl_hip_agent_begin_taught", "frirl_hip_agent_observe_taught", "frirl_hip_learn_demonstration"):
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES
    D = frirl_amd.DemonstrationDesc
    assert C.sizeof(D) == 72 and D.agent_stride.offset == 8 and D.obs.offset == 16 and D.action.offset == 32 and D.length.offset == 64
    assert callable(frirl_amd.learn_demonstration) and frirl_amd.Demonstration is not None
    import inspect
    assert "teacher" in inspect.signature(frirl_amd.agent_begin).parameters and "teacher" in inspect.signature(frirl_amd.agent_observe).parameters


def test_taught_calls_check_arguments_before_the_device(lib):
    import torch
    observe, begin = lib.frirl_hip_agent_observe_taught, lib.frirl_hip_agent_begin_taught
    for nant, A, what in ((1, 3, b"nant"), (9, 3, b"nant"), (4, 33, b"A=33")):
        keep, t, b, ag, ev, io = _valid_call(nant, A)
        addr = b.rb
        for teacher in (None, addr):
            assert observe(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io), teacher, None) == -2
            assert what in lib.frirl_hip_last_error(), lib.frirl_hip_last_error()
            assert begin(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io), teacher, None) == -2
    keep, t, b, ag, ev, io = _valid_call(4, 5)
    io.reward = None
    assert observe(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io), b.rb, None) == -2 and b"reward" in lib.frirl_hip_last_error()
    assert b"frirl_hip_agent_observe_taught" in lib.frirl_hip_last_error()
    if not torch.cuda.is_available():
        for nant, A in ((2, 1), (4, 5), (8, 32)):
            keep, t, b, ag, ev, io = _valid_call(nant, A)
            for teacher in (None, b.rb):
                assert observe(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io), teacher, None) == -1
                assert b"no CPU fallback" in lib.frirl_hip_last_error()
                assert begin(C.byref(t), C.byref(b), C.byref(ag), C.byref(ev), C.byref(io), teacher, None) == -1


def _valid_demo(nant=4, A=5, T=10):
    keep, t, b, ag, ev, io = _valid_call(nant, A)
    addr = b.rb
    dm = frirl_amd.DemonstrationDesc(T, T, addr, None, addr, addr, addr, None, None)
    return keep, t, b, ag, ev, dm


def test_learn_demonstration_checks_arguments_before_the_device(lib):
    import torch
    learn = lib.frirl_hip_learn_demonstration

    def call(t, b, ag, ev, dm, passes=1):
        return learn(C.byref(t), C.byref(b), C.byref(ag) if ag is not None else None, C.byref(ev), C.byref(dm) if dm is not None else None, passes,
                     None, None, None)

    keep, t, b, ag, ev, dm = _valid_demo()
    assert call(t, b, ag, ev, None) == -2 and b"NULL demo" in lib.frirl_hip_last_error()
    for field in ("obs", "action", "reward", "success"):
        keep, t, b, ag, ev, dm = _valid_demo()
        setattr(dm, field, None)
        assert call(t, b, ag, ev, dm) == -2 and b"NULL" in lib.frirl_hip_last_error(), field
    for T in (0, -3):
        keep, t, b, ag, ev, dm = _valid_demo()
        dm.T = T
        assert call(t, b, ag, ev, dm) == -2 and b"T=" in lib.frirl_hip_last_error()
    for passes in (0, -1, 1025):
        keep, t, b, ag, ev, dm = _valid_demo()
        assert call(t, b, ag, ev, dm, passes) == -2 and b"passes" in lib.frirl_hip_last_error()
    for stride in (-1, 1, 9):
        keep, t, b, ag, ev, dm = _valid_demo(T=10)
        dm.agent_stride = stride
        assert call(t, b, ag, ev, dm) == -2 and b"agent_stride" in lib.frirl_hip_last_error()
    # the checks of the agent calls
    for nant, A, what in ((1, 3, b"nant"), (9, 3, b"nant"), (4, 33, b"A=33")):
        keep, t, b, ag, ev, dm = _valid_demo(nant, A)
        assert call(t, b, ag, ev, dm) == -2 and what in lib.frirl_hip_last_error()
    keep, t, b, ag, ev, dm = _valid_demo()
    b.maxR = 9            # the sweeps read rules in 16-byte pairs: an odd capacity is refused, so a pair never leaves its column
    assert call(t, b, ag, ev, dm) == -2 and b"even" in lib.frirl_hip_last_error()
    keep, t, b, ag, ev, dm = _valid_demo()
    ag.grid_len[1] = 0
    assert call(t, b, ag, ev, dm) == -2 and b"grid_len" in lib.frirl_hip_last_error()
    keep, t, b, ag, ev, dm = _valid_demo()
    assert call(t, b, None, ev, dm) == -2
    keep, t, b, ag, ev, dm = _valid_demo()
    ev.done = None
    assert call(t, b, ag, ev, dm) == -2 and b"env state" in lib.frirl_hip_last_error()
    if not torch.cuda.is_available():       # valid arguments: no CPU fallback, the device check answers
        for nant, A, stride, passes in ((2, 1, 10, 1), (4, 5, 0, 1024), (8, 32, 4096, 2)):
            keep, t, b, ag, ev, dm = _valid_demo(nant, A)
            dm.agent_stride = stride
            assert call(t, b, ag, ev, dm, passes) == -1
            assert b"no CPU fallback" in lib.frirl_hip_last_error()
