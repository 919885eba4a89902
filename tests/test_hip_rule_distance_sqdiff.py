"""The squared-difference form of the packed rule-distance scan (option rd_sqdiff, shipped): per-workgroup LDS tables of
(q_k - ve[k][i])^2 and a short square root when every table entry is 0 or within [2^-767, 2^1000], else __dsqrt_rn.
Bit-identical to the scan without the tables (rd_sqdiff = 0), the 16-bit mirror (rd_packed = 0), the observation pre-pass
(rd_qpass = 1) and the oracle, also on tables that force the __dsqrt_rn fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

import frirl_amd
from tests.problems import Batch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sqrt_pair(a):
    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    fast, ref = torch.empty_like(a), torch.empty_like(a)
    rc = frirl_amd.lib().five_hip_sqrt_unscaled_check(C.c_void_p(a.data_ptr()), C.c_void_p(fast.data_ptr()), C.c_void_p(ref.data_ptr()),
                                                      a.numel(), None)
    frirl_amd.check(rc, "five_hip_sqrt_unscaled_check")
    torch.cuda.synchronize()
    return fast.cpu().numpy(), ref.cpu().numpy()


def guard(prob, x):
    ok = torch.empty((prob.E,), dtype=torch.int32, device=x.device)
    rc = frirl_amd.lib().five_hip_rule_distance_sq_guard(C.byref(prob.tables), prob.E, C.c_void_p(x.data_ptr()), C.c_void_p(ok.data_ptr()), None)
    frirl_amd.check(rc, "five_hip_rule_distance_sq_guard")
    torch.cuda.synchronize()
    return ok.cpu().numpy()


@pytest.mark.gpu
def test_short_sqrt_matches_dsqrt_rn():
    rng = np.random.default_rng(7)
    lo = np.ldexp(1.0, -767)
    edge = [0.0, lo, np.nextafter(lo, np.inf), np.nextafter(np.nextafter(lo, np.inf), np.inf), 1.0, 2.0, 0.25, np.ldexp(1.0, 1000),
            np.nextafter(np.ldexp(1.0, 1000), 0.0), np.ldexp(1.0, 1020), np.finfo(np.float64).max]
    n = 1 << 20
    rand = np.ldexp(1.0 + rng.random(n), rng.integers(-767, 1021, n))                         # random mantissas and exponents
    near_pow2 = np.ldexp(1.0, rng.integers(-766, 1020, 4096))
    near_pow2 = np.concatenate([near_pow2, np.nextafter(near_pow2, 0.0), np.nextafter(near_pow2, np.inf)])
    k = rng.integers(1, 1 << 26, 1 << 16).astype(np.float64)
    squares = np.concatenate([k * k, np.ldexp(k * k, 2 * rng.integers(-300, 400, k.size)), np.arange(1, 4097, dtype=np.float64) ** 2])
    near_sq = np.concatenate([np.nextafter(squares, 0.0), np.nextafter(squares, np.inf)])
    sums = (rng.random((n // 4, 5)) ** 2).sum(1)                                           # sums of squares as the scan makes them
    a = np.concatenate([edge, rand, near_pow2, squares, near_sq, sums])
    assert ((a == 0.0) | ((a >= lo) & np.isfinite(a))).all()
    fast, ref = sqrt_pair(a)
    bad = np.nonzero(bits(fast) != bits(ref))[0]
    assert bad.size == 0, [(a[i], fast[i], ref[i]) for i in bad[:5]]
    assert (bits(ref) == bits(np.sqrt(a))).all()                                           # both correctly rounded


def problem(nant, U, R, E, seed, tables=None):
    b = Batch(nant, U, R, E, A=0, seed=seed, ragged=True, maxR=R + (R & 1) + 34, tables=tables)
    x = b.queries(seed=seed + 1, hit_fraction=0.5)
    return b, x


def scans(b, x, hip_option):
    """(ruledists, hit) of every variant of the scan on the same problem, and the oracle."""
    prob = b.to_device(compressed=True)
    assert prob.pidx is not None
    xd = torch.from_numpy(x).cuda()
    out = {}

    def run(name):
        d, hit = prob.rule_distance(xd)
        torch.cuda.synchronize()
        out[name] = (d.cpu().numpy(), hit.cpu().numpy().astype(np.int64))

    run("sqdiff")
    _, hit_only = prob.rule_distance(xd, materialise=False)
    torch.cuda.synchronize()
    assert (hit_only.cpu().numpy() == out["sqdiff"][1]).all(), "NULL ruledists"
    hip_option("rd_qpass", 1)
    run("qpass")
    hip_option("rd_qpass", 0)
    for un in (4, 2):
        hip_option("rd_unroll", un)
        run(f"unroll{un}")
    hip_option("rd_unroll", 0)
    hip_option("rd_sqdiff", 0)
    run("no_sqdiff")
    hip_option("rd_sqdiff", 1)
    hip_option("rd_packed", 0)
    run("mirror16")
    hip_option("rd_packed", 1)
    d_ref, hit_ref = b.oracle_rule_distance(x)
    return prob, xd, out, (d_ref, hit_ref.astype(np.int64))


def assert_all_same(b, out, ref):
    d_ref, hit_ref = ref
    d0 = out["no_sqdiff"][0]
    for name, (d, hit) in out.items():
        assert (hit == hit_ref).all(), (name, hit, hit_ref)
        for e in range(b.E):
            n = int(b.nrules[e])
            assert (bits(d[e, :n]) == bits(d_ref[e, :n])).all(), (name, "vs oracle", e)
            m = min(n + (n & 1), b.maxR)                                  # the odd tail's pair column is written too
            if name != "mirror16":
                assert (bits(d[e, :m]) == bits(d0[e, :m])).all(), (name, "vs rd_sqdiff=0", e)


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("R", [4097, 1531])
def test_sqdiff_scan_bit_identical(nant, R, hip_option):
    b, x = problem(nant, 41, R, 7, seed=60 + nant * 3 + R % 7)
    prob, xd, out, ref = scans(b, x, hip_option)
    assert (guard(prob, xd) == 1).all(), "synthetic tables should take the short square root"
    assert_all_same(b, out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("nant,U", [(3, 64), (6, 41), (8, 64)])
def test_sqdiff_scan_bit_identical_wide(nant, U, hip_option):
    b, x = problem(nant, U, 2049, 5, seed=nant + U)
    _, _, out, ref = scans(b, x, hip_option)
    assert_all_same(b, out, ref)


def scaled_tables(nant, U, seed, scale):
    rng = np.random.default_rng(seed)
    u = np.tile(np.linspace(-1.0, 1.0, U), (nant, 1))
    ve = scale * (1.0 + rng.random((nant, U)))
    return u, ve


@pytest.mark.gpu
@pytest.mark.parametrize("nant", [2, 5])
@pytest.mark.parametrize("scale,what", [(np.ldexp(1.0, -400), "tiny"), (1e200, "overflow")])
def test_sqdiff_fallback_bit_identical(nant, scale, what, hip_option):
    """VE values near 2^-400 make squares below 2^-767; near 1e200 the squares overflow to inf.  Either way the workgroup's guard
    fails, the scan falls back to __dsqrt_rn, and every variant keeps the oracle's bits (inf distances included)."""
    b, x = problem(nant, 41, 3001, 6, seed=90 + nant, tables=scaled_tables(nant, 41, 5 + nant, scale))
    prob, xd, out, ref = scans(b, x, hip_option)
    assert (guard(prob, xd) == 0).all(), "these tables must take the __dsqrt_rn fallback"
    d = out["sqdiff"][0]
    n0 = int(b.nrules[0])
    if what == "tiny":
        assert ((d[0, :n0] > 0.0) & (d[0, :n0] < np.ldexp(1.0, -380))).any()
    else:
        assert np.isinf(d[0, :n0]).any()
    assert (out["sqdiff"][1] >= 0).any(), "expected exact hits"
    assert_all_same(b, out, ref)
