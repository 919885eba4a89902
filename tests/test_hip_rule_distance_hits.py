"""Exact hits of the coded rule-distance scan (rule_distance_cd_kernel): the sweep only keeps a per-lane minimum, and a wave that saw a
zero decodes its codes again, takes the lowest hitting rule per lane, reduces over the wave and issues one atomicMin.  Rule bases of
tests/test_hip_rule_distance_coded.py (nant 5 and 3, U 41, maxR 4098, E 9 with its rule counts) with hits planted where that path can
go wrong; distances and hit index are held bit for bit to the oracle and to the 4-byte route (rd_coded = 0).  A thread owns rules
2 t + p + 512 j of a 2048-rule tile (p < 2, j < 4), a wave 64 consecutive threads.

Two sets of observations on the same rule bases (environment: planted columns -> wanted hit; counts 4098, 1, 2, 33, 2047, 2048, 2049,
4095, 4097; environment 7 takes the __dsqrt_rn branch):
  set a   0: 1500, 3000, 4097 (three tiles, duplicated antecedents) -> 1500    1: partner column 1 of the odd last rule alone -> -1
          2: 0, 1 (one pair) -> 0         3: 9, 30 (two lanes of a wave) -> 9   4: partner column 2047 alone -> -1
          5: 700, 1213 (one lane, pairs 512 apart) -> 700                       6: 2048 and its partner column 2049 -> 2048
          7: 2100, 2400 (two waves of a tile, __dsqrt_rn) -> 2100               8: 1234 and partner column 4097 -> 1234
  set b   0: 2148, 2348 (two waves of a tile) -> 2148     1: 0 and partner column 1 -> 0     2: nothing -> -1
          3: 32 and partner column 33 -> 32               4: 2046 and partner column 2047 -> 2046
          5: 2046, 2047 (one pair) -> 2046                6: 5, 517, 2048 (one lane twice, and another tile) -> 5
          7: partner column 4095 alone (__dsqrt_rn) -> -1                       8: 4096, 100 (two tiles) -> 100

Mutations tried on a scratch build, and what failed under each (test_scan_bit_identical is the test of
tests/test_hip_rule_distance_coded.py; everything passes on the shipped build):
  the rare path takes the highest index of a lane instead of the lowest: test_hits[5-a], [5-b], [3-a], [3-b] and
      test_hits_without_distances[5], [3] -- environments 2 and 5 of set a (1 and 1213 for 0 and 700), 5 and 6 of set b (2047 and 517
      for 2046 and 5); test_scan_bit_identical passed (it has one hit per environment)
  the rare path drops the `rr + 1 < R` bound of the partner column: all six of the above (the partner columns of set a's environments
      1 and 4 and set b's 7 become hits) and test_scan_bit_identical[5], [3]
  sqrt_unscaled returns r unguarded (no maximum with 0): test_hits[5-a], [5-b], [3-a], [3-b] and test_scan_bit_identical[5], [3] (NaN
      distances of the hitting rules); test_hits_without_distances passed, as no distance is written there"""
import numpy as np
import pytest
import torch

from tests.test_hip_rule_distance_coded import COUNTS, SLOW, assert_same, coded_case, run, workspace_views

SETS = {
    "a": {0: ([1500, 3000, 4097], 1500), 1: ([1], -1), 2: ([0, 1], 0), 3: ([9, 30], 9), 4: ([2047], -1), 5: ([700, 1213], 700),
          6: ([2048, 2049], 2048), 7: ([2100, 2400], 2100), 8: ([1234, 4097], 1234)},
    "b": {0: ([2148, 2348], 2148), 1: ([0, 1], 0), 2: ([], -1), 3: ([32, 33], 32), 4: ([2046, 2047], 2046), 5: ([2046, 2047], 2046),
          6: ([5, 517, 2048], 5), 7: ([4095], -1), 8: ([4096, 100], 100)},
}
_cache = {}


def plant(b, rng, e, cols, first=None):
    """Writes one antecedent vector that no other column of rule base e has into the columns `cols`; returns the observation on it."""
    keep = np.ones(b.maxR, dtype=bool)
    keep[cols] = False
    others = b.uidx[e][:, keep]
    while True:
        cand = np.array([rng.integers(0, 41) for _ in range(b.nant - 1)] + [20 * rng.integers(0, 3)], dtype=b.uidx.dtype)
        if first is not None:
            cand[0] = first
        elif cand[0] in (2, 3):                  # the table entries that take an observation out of the short square root's range
            continue
        if not (others == cand[:, None]).all(0).any():
            break
    for r in cols:
        b.uidx[e, :, r] = cand
        b.rb[e, :b.nant, r] = b.ve[np.arange(b.nant), cand]
    return b.u[np.arange(b.nant), cand]


def hits_case(nant, name):
    """(batch, x, wanted hits, oracle result) of one set, built once: a private copy of the coded test's rule bases with the set's columns
    planted.  Environment SLOW observes grid point 2 of dimension 0 (squares to 2^-800 against entry 3: the __dsqrt_rn branch)."""
    if (nant, name) in _cache:
        return _cache[nant, name]
    b0 = coded_case(nant)[0]
    b = type(b0).__new__(type(b0))
    b.__dict__.update(b0.__dict__)
    b.uidx, b.rb = b0.uidx.copy(), b0.rb.copy()
    assert list(b.nrules) == COUNTS
    x = b.queries(seed=21, hit_fraction=0.0, hit_last=False)
    x[SLOW, 0] = b.u[0, 2]
    rng = np.random.default_rng(100 * nant + ord(name))
    want = np.full(b.E, -1, dtype=np.int32)
    for e, (cols, hit) in SETS[name].items():
        want[e] = hit
        if cols:
            x[e] = plant(b, rng, e, cols, first=2 if e == SLOW else None)
    ref = b.oracle_rule_distance(x)
    assert (ref[1] == want).all(), (ref[1], want)                # the cases are what they claim to be
    for e, (cols, hit) in SETS[name].items():                    # every planted column is at distance 0, rule or partner column
        real = [r for r in cols if r < b.nrules[e]]
        assert (ref[0][e, real] == 0.0).all() and (np.count_nonzero(ref[0][e, :b.nrules[e]] == 0.0) == len(real))
    _cache[nant, name] = (b, x, want, ref)
    return _cache[nant, name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("nant", [5, 3])
def test_hits(nant, name, hip_option):
    b, x, want, ref = hits_case(nant, name)
    prob = b.to_device(compressed=True)
    assert prob.codes is not None and list(prob._code_d) == [41] * (nant - 1) + [3]
    xd = torch.from_numpy(x).cuda()
    coded = run(prob, xd)
    _, fast = workspace_views(prob)
    hip_option("rd_coded", 0)
    plain = run(prob, xd)
    hip_option("rd_coded", 1)
    print("hits", nant, name, coded[1].tolist(), plain[1].tolist(), want.tolist())
    assert fast[SLOW] == 0 and fast.sum() == b.E - 1, fast      # one environment on __dsqrt_rn, eight on the short square root
    assert (coded[1] == want).all(), (coded[1], want)
    assert_same(b, coded, ref, False, "vs oracle")
    assert_same(b, coded, plain, True, "vs rd_coded=0")
    for e, (cols, _) in SETS[name].items():                     # the partner column of an odd last rule is written, and is 0.0 where planted
        for r in cols:
            if r < min(b.nrules[e] + (b.nrules[e] & 1), b.maxR):
                assert coded[0][e, r] == 0.0 and not np.signbit(coded[0][e, r]), (e, r)


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [5, 3])
def test_hits_without_distances(nant, hip_option):
    """ruledists = None (the WRITE = false instantiation) with hits: the same indices on both routes."""
    for name in ("a", "b"):
        b, x, want, _ = hits_case(nant, name)
        prob = b.to_device(compressed=True)
        xd = torch.from_numpy(x).cuda()
        d, hit = run(prob, xd, materialise=False)
        hip_option("rd_coded", 0)
        _, hit0 = run(prob, xd, materialise=False)
        hip_option("rd_coded", 1)
        assert d is None and (hit == want).all() and (hit0 == want).all(), (name, hit, hit0, want)
