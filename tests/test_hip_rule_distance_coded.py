"""The coded rule-distance scan (option rd_coded, five_hip_rule_distance_coded_ws): 3-byte dictionary codes in lane-tiled words.
Distances and hit indices are held bit for bit to the oracle and to the 4-byte packed route (rd_coded = 0), the pack kernel to
the NumPy model of tests/test_rd_codes_host.py byte for byte, and the workspace tables to their digit-space definition (which
also shows which route ran).

Mutations of rule_distance_cd_kernel tried on a scratch build, and the tests of this file that failed under each (the other four
passed; all seven pass on the shipped build):
  `>> 17` for `>> 18` in the decode of a pair field        test_scan_bit_identical[5], [3], test_edit_in_place_repacks
  pieces 1 and 2 of a lane swapped in the loads            test_scan_bit_identical[5], [3], test_edit_in_place_repacks
  environment stride one tile short (cpe - 1 tiles)        test_scan_bit_identical[5], [3], test_edit_in_place_repacks
tests/test_rd_codes_host.py::test_shift_17_is_not_a_division shows the first one in the arithmetic alone."""
from ctypes import c_int32 as C_int32

import numpy as np
import pytest
import torch

import frirl_amd
from tests.problems import Batch
from tests.test_rd_codes_host import TILE, dictionaries, encode, field_params, tile_layout

TS = 64
MAXR = 4098                                  # three tiles, the last one holding two rules
COUNTS = [MAXR, 1, 2, 33, 2047, 2048, 2049, 4095, 4097]      # E = 9: not a multiple of the 8-environment XCD group
SLOW = 7                                     # the environment whose observation leaves the range of the short square root


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def edge_tables(nant, U):
    """VE values in [1, 2) except ve[0][2] = 0.0 and ve[0][3] = 2^-400: an observation on grid point 2 of dimension 0 squares to
    2^-800 against entry 3, below the 2^-767 the short square root needs."""
    rng = np.random.default_rng(11)
    u = np.tile(np.linspace(-1.0, 1.0, U), (nant, 1))
    ve = 1.0 + rng.random((nant, U))
    ve[0, 2], ve[0, 3] = 0.0, np.ldexp(1.0, -400)
    return u, ve


def on_rule(b, e, r):
    return b.u[np.arange(b.nant), b.uidx[e, :, r]]


def make_unique(b, rng, e, r):
    """Gives column r of environment e antecedents that no other column of that rule base has (same index sets per dimension)."""
    others = np.delete(b.uidx[e], r, axis=1)
    while True:
        cand = np.array([rng.integers(0, 41) for _ in range(b.nant - 1)] + [20 * rng.integers(0, 3)], dtype=b.uidx.dtype)
        if not (others == cand[:, None]).all(0).any():
            break
    b.uidx[e, :, r] = cand
    b.rb[e, :b.nant, r] = b.ve[np.arange(b.nant), cand]


_cache = {}


def coded_case(nant):
    """(batch, x, wanted hits, oracle result), built once per nant: full rule bases cut to COUNTS (so the columns at and beyond
    nrules hold real antecedents), U 41 with a 3-value action dimension."""
    if nant in _cache:
        return _cache[nant]
    E = len(COUNTS)
    b = Batch(nant, 41, MAXR, E, A=3, seed=40 + nant, ragged=False, tables=edge_tables(nant, 41))
    b.nrules = np.array(COUNTS, dtype=np.int32)
    x = b.queries(seed=9, hit_fraction=0.0, hit_last=False)
    want = {0: 4097,       # last rule of the nearly empty third tile (odd index)
            2: 0,          # first rule of the first tile
            3: 32,         # odd rule count: the last rule has no partner
            5: 2047,       # last rule of a tile
            6: 2048,       # first rule of a tile, and an odd last rule
            8: 4096}       # first rule of the third tile
    rng = np.random.default_rng(17 + nant)
    for e, r in list(want.items()) + [(4, 2047)]:
        make_unique(b, rng, e, r)
        x[e] = on_rule(b, e, r)              # e = 4, nrules 2047: column 2047 is scanned as rule 2046's partner and must NOT hit
    x[SLOW, 0] = b.u[0, 2]
    ref = b.oracle_rule_distance(x)
    for e, r in list(want.items()) + [(4, -1)]:      # the cases are what they claim to be
        assert ref[1][e] == r, (e, ref[1][e])
    _cache[nant] = (b, x, want, ref)
    return _cache[nant]


def run(prob, xd, **kw):
    d, hit = prob.rule_distance(xd, **kw)
    torch.cuda.synchronize()
    return (d.cpu().numpy() if d is not None else None), hit.cpu().numpy()


def workspace_views(prob):
    ws = prob._rd_workspace(None)
    n = prob.E * prob.nant * TS * 8
    return ws[:n].view(torch.float64).reshape(prob.E, prob.nant, TS).cpu().numpy(), ws[n:n + 4 * prob.E].view(torch.int32).cpu().numpy()


def assert_same(b, got, ref, upto_pair, what):
    (d, hit), (d_ref, hit_ref) = got, ref
    assert (hit == hit_ref).all(), (what, hit, hit_ref)
    for e in range(b.E):
        n = int(b.nrules[e])
        m = min(n + (n & 1), b.maxR) if upto_pair else n
        assert (bits(d[e, :m]) == bits(d_ref[e, :m])).all(), (what, e)


def model(b):
    uidx = b.uidx.astype(np.uint16)
    dicts = dictionaries(uidx, b.nrules)
    fields = field_params([len(x) for x in dicts])
    return dicts, fields, (tile_layout(encode(uidx, b.nrules, dicts, fields)) if fields else None)


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [5, 3])
def test_scan_bit_identical(nant, hip_option):
    b, x, want, ref = coded_case(nant)
    prob = b.to_device(compressed=True)
    assert prob.codes is not None and list(prob._code_d) == [41] * (nant - 1) + [3]
    xd = torch.from_numpy(x).cuda()
    coded = run(prob, xd)
    sqtab, fast = workspace_views(prob)
    _, hit_only = run(prob, xd, materialise=False)
    hip_option("rd_coded", 0)
    plain = run(prob, xd)
    sqtab0, fast0 = workspace_views(prob)
    _, hit_only0 = run(prob, xd, materialise=False)
    hip_option("rd_coded", 1)

    assert_same(b, coded, ref, False, "vs oracle")
    assert_same(b, coded, plain, True, "vs rd_coded=0")
    assert (hit_only == coded[1]).all() and (hit_only0 == coded[1]).all()
    assert coded[1][4] == -1 and all(coded[1][e] == r for e, r in want.items())
    # the square-root branch: one environment on __dsqrt_rn beside eight on the short form, on both routes
    for tab, flag in ((sqtab, fast), (sqtab0, fast0)):
        ok = ((tab == 0.0) | ((tab >= np.ldexp(1.0, -767)) & (tab <= np.ldexp(1.0, 1000)))).all((1, 2))
        assert (flag == ok).all() and flag[SLOW] == 0 and flag.sum() >= 3, flag
    # digit-space tables on the coded route (the action dimension's digits 0, 1, 2 are indices 0, 20, 40), index space on the other
    k = nant - 1
    assert (bits(sqtab[:, :k, :41]) == bits(sqtab0[:, :k, :41])).all()
    assert (bits(sqtab[:, k, :3]) == bits(sqtab0[:, k, [0, 20, 40]])).all()
    assert (bits(sqtab[:, k, 3:]) == bits(sqtab0[:, k, 41:42])).all()           # padding: table value 0.0
    assert (bits(sqtab[:, k, 1]) != bits(sqtab0[:, k, 1])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [5, 3])
def test_pack_matches_model(nant):
    b, _, _, _ = coded_case(nant)
    prob = b.to_device(compressed=True)
    torch.cuda.synchronize()
    dicts, fields, image = model(b)
    assert prob.codes.numel() == b.E * 3 * 3 * TILE == image.size
    assert list(prob._code_d) == [len(x) for x in dicts]
    dct = prob._code_dict.cpu().numpy()
    rank = prob._code_rank.cpu().numpy()
    for k in range(nant):
        assert (dct[k, :len(dicts[k])] == dicts[k]).all() and (dct[k, len(dicts[k]):] == 255).all()
        assert (rank[k, dicts[k]] == np.arange(len(dicts[k]))).all()
    got = prob.codes.cpu().numpy().reshape(b.E, -1)
    assert (got == image).all(), np.argwhere(got != image)[:8]


@pytest.mark.gpu
def test_wide_dictionaries_run_the_packed_route():
    """All 41 indices in five dimensions: 11 + 11 + 6 = 28 bits, no coded copy, the 4-byte route and the same results."""
    b = Batch(5, 41, 700, 5, A=0, seed=3, ragged=True, maxR=734)
    x = b.queries(seed=4, hit_fraction=0.5)
    assert [len(v) for v in dictionaries(b.uidx.astype(np.uint16), b.nrules)] == [41] * 5
    d = (C_int32 * 5)(*([41] * 5))
    assert frirl_amd.lib().five_hip_rule_distance_coded_bytes(5, 41, b.E, b.maxR, d) == 0
    prob = b.to_device(compressed=True)
    assert prob.pidx is not None and prob.codes is None
    xd = torch.from_numpy(x).cuda()
    got = run(prob, xd)
    assert_same(b, got, b.oracle_rule_distance(x), False, "vs oracle")
    sqtab, _ = workspace_views(prob)
    assert (sqtab[:, :, 41:] == sqtab[:, :, 41:42]).all()                        # index-space tables: entries 41.. are padding


def test_coded_bytes():
    L = frirl_amd.lib()
    arr = lambda *v: (C_int32 * len(v))(*v)                                      # noqa: E731
    assert L.five_hip_rule_distance_coded_bytes(5, 41, 8192, 65792, arr(41, 41, 41, 41, 3)) == 8192 * 33 * 6144
    assert L.five_hip_rule_distance_coded_bytes(3, 41, 9, 4098, arr(41, 41, 3)) == 9 * 3 * 6144
    assert L.five_hip_rule_distance_coded_bytes(5, 41, 9, 4098, arr(41, 41, 41, 41, 41)) == 0        # 28 bits
    assert L.five_hip_rule_distance_coded_bytes(4, 64, 9, 4098, arr(64, 64, 64, 64)) == 9 * 3 * 6144  # 12 + 12
    assert L.five_hip_rule_distance_coded_bytes(5, 64, 9, 4098, arr(64, 64, 64, 64, 2)) == 0
    assert L.five_hip_rule_distance_coded_bytes(6, 41, 9, 4098, arr(2, 2, 2, 2, 2, 2)) == 0           # nant > 5
    assert L.five_hip_rule_distance_coded_bytes(5, 65, 9, 4098, arr(2, 2, 2, 2, 2)) == 0              # not a packed shape
    assert L.five_hip_rule_distance_coded_bytes(3, 41, 9, 4098, arr(41, 0, 3)) == 0
    assert L.five_hip_rule_distance_coded_bytes(3, 41, 9, 4098, None) == 0


@pytest.mark.gpu
def test_edit_in_place_repacks():
    """A new index written into uidx in place: the next scan rebuilds the dictionaries and the copy, and is right."""
    b0, x0, _, _ = coded_case(3)
    b = Batch.__new__(Batch)
    b.__dict__.update(b0.__dict__)
    b.uidx, b.rb, x = b0.uidx.copy(), b0.rb.copy(), x0.copy()
    prob = b.to_device(compressed=True)
    xd = torch.from_numpy(x).cuda()
    before = run(prob, xd)
    assert list(prob._code_d) == [41, 41, 3]
    e, r = 8, 4095
    b.uidx[e, 2, r] = 7                                                          # the action dimension gains index 7
    b.rb[e, 2, r] = b.ve[2, 7]
    prob.uidx[e, 2, r] = 7
    prob.rb[e, 2, r] = float(b.ve[2, 7])
    x[e] = on_rule(b, e, r)
    xd = torch.from_numpy(x).cuda()
    ref = b.oracle_rule_distance(x)
    assert ref[1][e] == r
    got = run(prob, xd)
    assert list(prob._code_d) == [41, 41, 4]
    assert (prob._code_dict[2, :5].cpu().numpy() == [0, 7, 20, 40, 255]).all()
    assert_same(b, got, ref, False, "after the edit")
    assert got[1][e] == r and before[1][e] == 4096
    dicts, fields, image = model(b)
    assert (prob.codes.cpu().numpy().reshape(b.E, -1) == image).all()

