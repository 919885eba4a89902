"""Host side of the caller-stepped API for EVERY agent's own rule base (no GPU needed): the new ABI symbols and struct layout, and the
argument checks of frirl_hip_policy_batch_begin / _observe and frirl_hip_batch_reducer_create (EINVAL before ENODEV)."""
import ctypes as C

import pytest

import frirl_amd

NEW_SYMBOLS = ["frirl_hip_policy_batch_begin", "frirl_hip_policy_batch_observe", "frirl_hip_batch_reducer_create",
               "frirl_hip_batch_reducer_next_round", "frirl_hip_batch_reducer_begin", "frirl_hip_batch_reducer_observe",
               "frirl_hip_batch_reducer_end_round", "frirl_hip_batch_reducer_result", "frirl_hip_batch_reducer_row_done",
               "frirl_hip_batch_reducer_destroy"]


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    for n in ("PolicyBatchRows", "BatchReducer", "reduce_external_batch"):
        assert hasattr(frirl_amd, n), n
    assert hasattr(frirl_amd.Problem, "policy_batch_begin") and hasattr(frirl_amd.Problem, "policy_batch_observe")


def test_struct_layout_matches_the_header():
    """struct frirl_hip_policy_batch_rows on LP64: an int32 in front of a pointer is padded to 8 bytes."""
    P = frirl_amd.PolicyBatchRowsDesc
    want = dict(n=0, done=8, ep_steps=16, success=24, ep_reward=32, row_count=40, step_cap=48, agents=56, nagents=64, exclude_mask=72,
                rule_slot=80, rows_live=88)
    assert [f[0] for f in P._fields_] == list(want)
    for name, off in want.items():
        assert getattr(P, name).offset == off, name
    assert C.sizeof(P) == 96


def _valid_call(nant, A, E=3, n=4):
    buf = (C.c_double * 16384)()
    addr = (C.addressof(buf) + 15) & ~15
    t = frirl_amd.Tables(nant, 41, addr, addr)
    b = frirl_amd.RuleBases(E, 8, addr, addr)
    ag = frirl_amd.AgentDesc()
    ag.A, ag.env_kind, ag.max_steps, ag.grid_values, ag.action_ve = A, frirl_amd.ENV_EXTERNAL, 10, addr, addr
    for k in range(min(nant, frirl_amd.MAX_NANT)):
        ag.grid_len[k] = 3
    if 1 <= nant <= frirl_amd.MAX_NANT:
        ag.grid_len[nant - 1] = min(A, frirl_amd.MAX_GRID)
    rows = frirl_amd.PolicyBatchRowsDesc(n, addr, addr, addr, addr, None, None, None, 0, None, None, None)
    io = frirl_amd.AgentIO(addr, None, addr, addr, None, addr, None)
    return buf, t, b, ag, rows, io


def _both(lib, t, b, ag, rows, io):
    args = [C.byref(x) if x is not None else None for x in (t, b, ag, rows, io)] + [None]
    return lib.frirl_hip_policy_batch_begin(*args), lib.frirl_hip_policy_batch_observe(*args)


def test_policy_batch_argument_checks_before_the_device(lib):
    import torch
    cases = []

    def case(what, nant=4, A=5, **kw):
        keep, t, b, ag, rows, io = _valid_call(nant, A, **kw)
        cases.append((what, [keep, t, b, ag, rows, io]))
        return cases[-1][1]

    case(b"nant", nant=1)
    case(b"nant", nant=9)
    case(b"A=0", A=0)
    case(b"A=33", A=33)
    case(b"n=0", n=0)
    case(b"n=-3", n=-3)
    for field in ("done", "ep_steps", "success", "ep_reward"):
        setattr(case(b"row state")[4], field, None)
    c = case(b"go together")
    c[4].exclude_mask = c[2].rb                 # exclude_mask without rule_slot
    c = case(b"go together")
    c[4].rule_slot = c[2].rb
    for nagents in (0, 4, -1):                  # E = 3
        c = case(b"nagents")
        c[4].agents, c[4].nagents = c[2].rb, nagents
    case(b"NULL")[5].obs = None
    case(b"NULL")[5].action_out = None
    case(b"NULL")[3].grid_values = None
    case(b"grid_len")[3].grid_len[1] = 0
    case(b"action grid")[3].grid_len[3] = 4
    for what, (keep, t, b, ag, rows, io) in cases:
        rb, ro = _both(lib, t, b, ag, rows, io)
        assert ro == -2 and what in lib.frirl_hip_last_error(), (what, lib.frirl_hip_last_error())
        assert rb == -2, what
    for field in ("reward", "success"):         # observe alone needs the reward and the success flag
        keep, t, b, ag, rows, io = _valid_call(4, 5)
        setattr(io, field, None)
        args = [C.byref(x) for x in (t, b, ag, rows, io)] + [None]
        assert lib.frirl_hip_policy_batch_observe(*args) == -2 and b"reward" in lib.frirl_hip_last_error()
    keep, t, b, ag, rows, io = _valid_call(4, 5)
    assert _both(lib, t, b, None, rows, io) == (-2, -2) and _both(lib, t, b, ag, None, io) == (-2, -2) and _both(lib, t, b, ag, rows, None) == (-2, -2)
    if not torch.cuda.is_available():           # valid arguments, E > 1 included: no CPU fallback, the device check answers
        for nant, A, E in ((2, 1, 1), (4, 5, 3), (8, 32, 64)):
            keep, t, b, ag, rows, io = _valid_call(nant, A, E=E)
            assert _both(lib, t, b, ag, rows, io) == (-1, -1)
            assert b"no CPU fallback" in lib.frirl_hip_last_error()
            rows.agents, rows.nagents = b.rb, E
            rows.exclude_mask = rows.rule_slot = b.rb
            assert _both(lib, t, b, ag, rows, io) == (-1, -1)


def test_batch_reducer_create_argument_checks(lib):
    import torch
    create = lib.frirl_hip_batch_reducer_create

    def make(strategy=1, depth=0, nant=4, A=5, E=3, agent=True):
        keep, t, b, ag, rows, io = _valid_call(nant, A, E)
        return create(C.byref(t), C.byref(b), C.byref(ag) if agent else None, None, None, strategy, 0.0, depth, None)

    for kw, what in ((dict(strategy=3), b"strategy 3"), (dict(strategy=0), b"strategy 0"), (dict(depth=13), b"depth 13"), (dict(depth=-1), b"depth"),
                     (dict(agent=False), b"NULL agent"), (dict(nant=9), b"nant"), (dict(A=33), b"A=33")):
        assert make(**kw) is None
        assert what in lib.frirl_hip_last_error(), (kw, lib.frirl_hip_last_error())
    if not torch.cuda.is_available():
        for depth in (0, 1, 12):
            assert make(depth=depth) is None and b"no CPU fallback" in lib.frirl_hip_last_error()
    # the other calls refuse a NULL handle
    q = C.c_int32()
    res = frirl_amd.ReduceResult()
    assert lib.frirl_hip_batch_reducer_next_round(None, C.byref(q), None, None) == -2 and lib.frirl_hip_batch_reducer_begin(None, None) == -2
    assert lib.frirl_hip_batch_reducer_observe(None, None, None) == -2 and lib.frirl_hip_batch_reducer_end_round(None) == -2
    assert lib.frirl_hip_batch_reducer_result(None, None, C.byref(res)) == -2
    assert lib.frirl_hip_batch_reducer_row_done(None) is None
    lib.frirl_hip_batch_reducer_destroy(None)
