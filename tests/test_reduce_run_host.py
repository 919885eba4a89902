"""CPU-side checks of the one host driver of the batched reductions (ReduceRun, csrc/reduce_run.hip): the four entry points that run it
refuse the same bad arguments before the device is looked at, each under its own name and otherwise in the same words, and the depth
rule is written once."""
import ctypes as C
import re

import pytest

import frirl_amd
from tests.test_reduce_batch_host import demo_args

RW_MAX_DEPTH = 12                                       # csrc/reduce_walk.h
ENTRIES = ["frirl_hip_reduce_batch", "frirl_hip_reduce_batch_starts", "frirl_hip_batch_reducer_create", "frirl_hip_batch_reducer_create_starts"]
WITH_STARTS = {"frirl_hip_reduce_batch_starts", "frirl_hip_batch_reducer_create_starts"}
WITH_WORKSPACE = {"frirl_hip_reduce_batch": "frirl_hip_reduce_batch_workspace_bytes",
                  "frirl_hip_reduce_batch_starts": "frirl_hip_reduce_batch_starts_workspace_bytes"}


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def refusals(lib, name):
    """{refusal: (refused with FRIRL_HIP_EINVAL or a NULL handle, frirl_hip_last_error)} of one entry point; everything else about the
    call is valid, so that on a host without a GPU it would reach the device check."""
    buf, addr, t, b, ag = demo_args()
    n, depth0 = 4, 4
    res = (frirl_amd.ReduceResult * 3)()
    ws = addr + 4096
    need = {"frirl_hip_reduce_batch": lib.frirl_hip_reduce_batch_workspace_bytes(3, 3, 8, depth0),
            "frirl_hip_reduce_batch_starts": lib.frirl_hip_reduce_batch_starts_workspace_bytes(3, 3, 8, depth0, n)}.get(name, 0)

    def call(strategy=1, depth=depth0, max_steps=10, n=n, wsp=ws, nbytes=need):
        a = frirl_amd.AgentDesc.from_buffer_copy(ag)
        a.max_steps = max_steps
        st = frirl_amd.ReduceStarts(n, 0, addr, None)
        tb = (C.byref(t), C.byref(b), C.byref(a))
        if name == "frirl_hip_reduce_batch":
            bad = lib.frirl_hip_reduce_batch(*tb, None, None, None, strategy, 0.0, depth, None, res, wsp, nbytes, None) == -2
        elif name == "frirl_hip_reduce_batch_starts":
            bad = lib.frirl_hip_reduce_batch_starts(*tb, None, C.byref(st), None, strategy, 0.0, depth, None, res, None, wsp, nbytes, None) == -2
        elif name == "frirl_hip_batch_reducer_create":
            bad = not lib.frirl_hip_batch_reducer_create(*tb, None, None, strategy, 0.0, depth, None)
        else:
            bad = not lib.frirl_hip_batch_reducer_create_starts(*tb, None, None, C.byref(st), strategy, 0.0, depth, None)
        return bad, lib.frirl_hip_last_error()

    out = {"strategy 0": call(strategy=0), "strategy 3": call(strategy=3), "depth -1": call(depth=-1),
           "depth max + 1": call(depth=RW_MAX_DEPTH + 1), "max_steps -1": call(max_steps=-1)}
    if name in WITH_STARTS:
        out.update({"n 0": call(n=0), "n max + 1": call(n=frirl_amd.REDUCE_MAX_STARTS + 1)})
    if name in WITH_WORKSPACE:
        out.update({"workspace NULL": call(wsp=None), "workspace misaligned": call(wsp=ws + 8), "workspace short": call(nbytes=need - 16)})
    return out


@pytest.fixture(scope="module")
def seen(lib):
    return {name: refusals(lib, name) for name in ENTRIES}


def wording(name, message):
    """the message after "<entry point>: ", with what legitimately differs in the workspace refusal taken out: the address and the
    sizes (the workspaces of the two calls differ in size) and the name of the *_workspace_bytes function"""
    assert message.startswith(name.encode() + b": "), (name, message)
    rest = message[len(name) + 2:]
    if name in WITH_WORKSPACE and b"workspace" in rest:
        assert b"(" + WITH_WORKSPACE[name].encode() + b")" in rest, (name, message)
        rest = re.sub(rb"0x[0-9a-f]+", b"P", re.sub(rb"\d+ bytes", b"N bytes", rest.replace(WITH_WORKSPACE[name].encode(), b"F")))
    return rest


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_refuse_alike_before_the_device(seen, name):
    mine = seen[name]
    assert len(mine) == 5 + 2 * (name in WITH_STARTS) + 3 * (name in WITH_WORKSPACE)
    for what, (refused, message) in mine.items():
        assert refused and b"no CPU fallback" not in message, (name, what, message)
        for other in ENTRIES:
            if what in seen[other]:
                assert wording(other, seen[other][what][1]) == wording(name, message), (name, other, what)
    # the words name the argument refused
    for what, word in (("strategy 0", b"strategy 0 "), ("strategy 3", b"strategy 3 "), ("depth -1", b"depth -1 outside 0..12"),
                       ("depth max + 1", b"depth 13 outside 0..12"), ("max_steps -1", b"max_steps=-1"), ("n 0", b"n=0 start states outside 1..256"),
                       ("n max + 1", b"n=257 start states outside 1..256"), ("workspace NULL", b"workspace"), ("workspace misaligned", b"16-byte aligned"),
                       ("workspace short", b"needs")):
        if what in mine:
            assert word in mine[what][1], (name, what, mine[what][1])


def test_depth_rule_is_written_once(lib):
    for E in (1, 6, 7, 64, 2048, 2049):
        for A in (3, 4, 5, 21):
            assert lib.frirl_hip_reduce_batch_depth(E, A) == lib.frirl_hip_reduce_batch_starts_depth(E, A, 1), (E, A)
