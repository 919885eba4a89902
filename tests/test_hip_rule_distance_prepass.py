"""The per-call pre-pass of the packed rule-distance scan (option rd_prepass, five_hip_rule_distance_packed_ws): one kernel
builds every environment's table of squared differences (q_k - ve[k][i])^2, its short-square-root flag and the hit reset in a
caller-owned workspace, and the scan's workgroups copy their environment's table instead of rebuilding it.  The tables are
checked against float64 NumPy bit for bit, the scan against the per-workgroup form (rd_prepass = 0), the f64 layout and the
oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import frirl_amd
from tests.problems import Batch

TS = 64                      # table row stride of the packed form (2^6 entries)
LO, HI = np.ldexp(1.0, -767), np.ldexp(1.0, 1000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ws_bytes(nant, U, E):
    return frirl_amd.lib().five_hip_rule_distance_packed_workspace_bytes(nant, U, E)


def test_workspace_bytes():
    assert ws_bytes(5, 41, 8192) == 8192 * (5 * TS * 8 + 4)
    assert ws_bytes(1, 2, 1) == TS * 8 + 4
    assert ws_bytes(8, 64, 3) == 3 * (8 * TS * 8 + 4)
    assert ws_bytes(5, 65, 10) == 0 and ws_bytes(16, 41, 10) == 0 and ws_bytes(5, 41, 0) == 0      # not served by the packed form


def test_workspace_checked_before_any_device_work():
    """NULL, too small or misaligned workspace: FRIRL_HIP_EINVAL with a message, before the device is even looked at (the
    pointers below are never dereferenced)."""
    L = frirl_amd.lib()
    t = frirl_amd.Tables(5, 41, 4096, 4096)
    b = frirl_amd.RuleBases(3, 64, 4096, 4096, 4096)
    need = ws_bytes(5, 41, 3)
    for ws, n in ((None, need), (4096, need - 1), (4096, 0), (4104, need)):
        rc = L.five_hip_rule_distance_packed_ws(C.byref(t), C.byref(b), 4096, 4096, 4096, 4096, ws, n, None)
        assert rc == -2, (ws, n, rc)                                        # FRIRL_HIP_EINVAL
        assert b"workspace" in L.frirl_hip_last_error()


def workspace_views(prob, stream=None):
    """(sqtab [E][nant][64] float64, fast [E] int32) of the workspace the last scan on `stream` used."""
    ws = prob._rd_workspace(stream)
    n = prob.E * prob.nant * TS * 8
    return ws[:n].view(torch.float64).reshape(prob.E, prob.nant, TS).cpu().numpy(), ws[n:n + 4 * prob.E].view(torch.int32).cpu().numpy()


def host_snap(u, x):
    """snap_index of the library (reference src/inl/min.inl:71-92) for a finite x, in Python floats (IEEE double)."""
    U = len(u)
    div = (u[U - 1] - u[0]) / float(U - 1)
    low = int((x - u[0]) / div)
    if low < 0:
        return 0
    if low >= U:
        return U - 1
    if low + 1 >= U:
        return low
    return low if abs(u[low] - x) <= abs(u[low + 1] - x) else low + 1


def in_range(s):
    with np.errstate(invalid="ignore"):
        return (s == 0.0) | ((s >= LO) & (s <= HI))


def edge_tables(nant, U):
    """Ordinary VE values in [1, 2) except: dimension 0 holds 0.0 and 2^-400 (an observation on either makes squares of 2^-800,
    below 2^-767), the last dimension holds +-1.5 * 2^499 (an observation on one makes a square of 9 * 2^998 > 2^1000 against
    the other; every other observation stays below).  Which environments leave the range of the short square root therefore
    depends on their observation alone."""
    rng = np.random.default_rng(11)
    u = np.tile(np.linspace(-1.0, 1.0, U), (nant, 1))
    ve = 1.0 + rng.random((nant, U))
    ve[0, 2], ve[0, 3] = 0.0, np.ldexp(1.0, -400)
    ve[nant - 1, 6], ve[nant - 1, 7] = np.ldexp(1.5, 499), -np.ldexp(1.5, 499)
    return u, ve


@pytest.mark.gpu
@pytest.mark.parametrize("nant,U", [(5, 41), (2, 64), (3, 17)])
def test_prepass_tables_match_numpy(nant, U, hip_option):
    E = 13
    b = Batch(nant, U, 700, E, A=0, seed=21 + nant, ragged=True, maxR=734, tables=edge_tables(nant, U))
    x = b.queries(seed=5, hit_fraction=0.5)
    on = lambda k, j: b.u[k, j]                                                # noqa: E731  an observation exactly on grid point j
    x[3, 0] = on(0, 2)                      # q_0 = 0.0: entry 3 squares to 2^-800
    x[4, 0] = on(0, 3)                      # q_0 = 2^-400: entry 2 and the padding entries square to 2^-800
    x[5, nant - 1] = on(nant - 1, 6)        # 9 * 2^998 against entry 7
    x[6, nant - 1] = on(nant - 1, 7)
    x[7, 0], x[7, nant - 1] = on(0, 2), on(nant - 1, 7)
    x[8, nant - 1] = np.nan                 # a NaN observation: whichever index the snap yields, every variant uses the same
    prob = b.to_device(compressed=True)
    assert prob.pidx is not None
    xd = torch.from_numpy(x).cuda()
    hit = torch.full((E,), 12345, dtype=torch.int32, device="cuda")
    d, hit = prob.rule_distance(xd, hit=hit)
    torch.cuda.synchronize()
    sqtab, fast = workspace_views(prob)
    d, hit = d.cpu().numpy(), hit.cpu().numpy()

    vep = np.zeros((nant, TS))
    vep[:, :U] = b.ve                       # padding entries: table value 0.0
    want_fast = np.zeros(E, dtype=np.int32)
    for e in range(E):
        for k in range(nant):
            if np.isnan(x[e, k]):           # the conversion of NaN to an index is the device's; the row must be that of SOME grid point
                rows = [bits((b.ve[k, j] - vep[k]) * (b.ve[k, j] - vep[k])) for j in range(U)]
                assert any((bits(sqtab[e, k]) == r).all() for r in rows), (e, k)
                continue
            q = b.ve[k, host_snap(b.u[k], x[e, k])]
            dd = q - vep[k]
            assert (bits(sqtab[e, k]) == bits(dd * dd)).all(), (e, k)        # same subtract and multiply, no contraction
        want_fast[e] = int(in_range(sqtab[e]).all())
    assert (fast == want_fast).all(), (fast, want_fast)
    assert (fast[[3, 4, 5, 6, 7]] == 0).all() and fast.sum() >= 3, fast      # both branches in one launch

    # the hit words are reset by the pre-pass, and the scan keeps the bits of the per-workgroup form on both branches
    hip_option("rd_prepass", 0)
    d0, hit0 = prob.rule_distance(xd)
    torch.cuda.synchronize()
    d0, hit0 = d0.cpu().numpy(), hit0.cpu().numpy()
    assert (hit == hit0).all() and (hit == -1).any() and (hit >= 0).any() and not (hit == 12345).any()
    d_ref, hit_ref = b.oracle_rule_distance(x)
    for e in range(E):
        n = int(b.nrules[e])
        m = min(n + (n & 1), b.maxR)
        assert (bits(d[e, :m]) == bits(d0[e, :m])).all(), e
        if e != 8:
            assert (bits(d[e, :n]) == bits(d_ref[e, :n])).all() and hit[e] == hit_ref[e], e


def ragged_batch(nant, U, E, seed):
    """Every rule base full (4200 rules), then rule counts that meet every edge of a 4096- or 2048-rule item."""
    maxR = 4200
    b = Batch(nant, U, maxR, E, A=0, seed=seed, ragged=False)
    counts = [maxR, 0, 1, 777, 4095, 2047, 4096, 2049, 4097, 2048]
    b.nrules = np.array([counts[e % len(counts)] for e in range(E)], dtype=np.int32)
    if E == 1:
        b.nrules[0] = 4095
    x = b.queries(seed=seed + 1, hit_fraction=0.5)
    return b, x


def run(prob, xd, **kw):
    d, hit = prob.rule_distance(xd, **kw)
    torch.cuda.synchronize()
    return (d.cpu().numpy() if d is not None else None), hit.cpu().numpy()


def assert_same(b, got, ref, upto_pair, what):
    (d, hit), (d_ref, hit_ref) = got, ref
    assert (hit == hit_ref).all(), (what, hit, hit_ref)
    for e in range(b.E):
        n = int(b.nrules[e])
        m = min(n + (n & 1), b.maxR) if upto_pair else n
        assert (bits(d[e, :m]) == bits(d_ref[e, :m])).all(), (what, e)


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("E", [1, 7])
def test_ws_scan_bit_identical(nant, E, hip_option):
    U = (41, 64, 17, 33)[nant % 4]
    b, x = ragged_batch(nant, U, E, seed=100 + 10 * nant + E)
    prob = b.to_device(compressed=True)
    assert prob.pidx is not None and ws_bytes(nant, U, E) > 0
    xd = torch.from_numpy(x).cuda()
    pre = run(prob, xd)
    _, hit_only = run(prob, xd, materialise=False)                              # ruledists = NULL
    variants = {}
    for un, chunk in ((4, 0), (4, 4096), (2, 0)):                               # other item sizes of the pre-pass form
        hip_option("rd_unroll", un)
        hip_option("rd_chunk", chunk)
        variants[f"unroll{un}/chunk{chunk}"] = run(prob, xd)
    hip_option("rd_unroll", 0)
    hip_option("rd_chunk", 0)
    hip_option("rd_prepass", 0)
    per_wg = run(prob, xd)
    hip_option("rd_prepass", 1)
    f64 = run(b.to_device(compressed=False), xd)
    oracle = b.oracle_rule_distance(x)
    assert (hit_only == pre[1]).all()
    assert_same(b, pre, per_wg, True, "vs rd_prepass=0")
    assert_same(b, pre, f64, False, "vs f64 columns")
    assert_same(b, pre, oracle, False, "vs oracle")
    for name, v in variants.items():
        assert_same(b, v, per_wg, True, name)


@pytest.mark.gpu
def test_two_problems_alternate_on_two_streams():
    """Each (Problem, stream) pair has a workspace of its own: calls that overlap on two streams do not disturb each other."""
    ba, xa = ragged_batch(5, 41, 7, seed=301)
    bb, xb = ragged_batch(5, 41, 9, seed=302)
    pa, pb = ba.to_device(compressed=True), bb.to_device(compressed=True)
    xa_d, xb_d = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    ref_a, ref_b = ba.oracle_rule_distance(xa), bb.oracle_rule_distance(xb)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = {}
    for name, p in (("a", pa), ("b", pb)):
        for i in range(2):
            outs[name, i] = (torch.full((p.E, p.maxR), -1.0, dtype=torch.float64, device="cuda"), torch.full((p.E,), 777, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for it in range(6):
        i = it & 1
        pa.rule_distance(xa_d, ruledists=outs["a", i][0], hit=outs["a", i][1], stream=streams[i])
        pb.rule_distance(xb_d, ruledists=outs["b", 1 - i][0], hit=outs["b", 1 - i][1], stream=streams[1 - i])
    torch.cuda.synchronize()
    assert len(pa._rd_ws) == 2 and len(pb._rd_ws) == 2
    assert pa._rd_workspace(streams[0]).data_ptr() != pa._rd_workspace(streams[1]).data_ptr()
    for i in range(2):
        assert_same(ba, (outs["a", i][0].cpu().numpy(), outs["a", i][1].cpu().numpy()), ref_a, False, ("a", i))
        assert_same(bb, (outs["b", i][0].cpu().numpy(), outs["b", i][1].cpu().numpy()), ref_b, False, ("b", i))


@pytest.mark.gpu
def test_bad_workspace_launches_nothing():
    b, x = ragged_batch(5, 41, 3, seed=77)
    prob = b.to_device(compressed=True)
    xd = torch.from_numpy(x).cuda()
    d = torch.full((prob.E, prob.maxR), -7.0, dtype=torch.float64, device="cuda")
    hit = torch.full((prob.E,), 4242, dtype=torch.int32, device="cuda")
    need = ws_bytes(5, 41, 3)
    ws = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    L = frirl_amd.lib()
    for wptr, n in ((None, need), (P(ws), need - 1)):
        rc = L.five_hip_rule_distance_packed_ws(C.byref(prob.tables), C.byref(prob._bases), P(prob.pidx), P(xd), P(d), P(hit), wptr, n, None)
        assert rc == -2 and b"workspace" in L.frirl_hip_last_error()
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == 4242).all() and (d.cpu().numpy() == -7.0).all() and (ws.cpu().numpy() == 0).all()
    rc = L.five_hip_rule_distance_packed_ws(C.byref(prob.tables), C.byref(prob._bases), P(prob.pidx), P(xd), P(d), P(hit), P(ws), need, None)
    frirl_amd.check(rc, "five_hip_rule_distance_packed_ws")
    torch.cuda.synchronize()
    assert_same(b, (d.cpu().numpy(), hit.cpu().numpy()), b.oracle_rule_distance(x), False, "exact workspace size")
