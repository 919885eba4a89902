"""Inputs and the high-precision reference of the Shepard weight w = s^(-p/2) (s = squared distance), shared by the CPU test of the
oracle's chain (tests/test_oracle_golden.py) and the GPU probe test (tests/test_hip_power.py).

The exact value comes from Python's `decimal` at 60 digits (Decimal(float) is exact; sqrt, divide and multiply are correctly rounded
to 60 digits: relative error < 1e-58 after 16 products).  It is kept as a double-double (hi + lo) so that the comparison is plain
numpy: for a computed w within a factor 2 of hi, w - hi is exact in double."""
import decimal
import functools

import numpy as np

from oracle import binding as ob

POWERS = tuple(range(1, 17))
DEMO_ENVS = ("mountaincar", "cartpole", "acrobot")


def bound(p):
    """Relative error bound of every weight form: p x 4e-16.  Derived, not measured: the refined y = s^(-1/2) is good to 1.7e-16
    (csrc/sweeps.h), raising it to p multiplies that by p, each of the p - 1 products rounds once (<= 1.1e-16): less than p x 2.8e-16,
    rounded up."""
    return p * 4e-16


@functools.lru_cache(maxsize=None)
def inputs():
    """About 20 000 squared distances: log-uniform in [2^-60, 2^12]; every power of two there with two neighbours on each side; the
    squared VE differences of the three demo tables; a few hundred log-uniform in [2^-120, 2^120]."""
    rng = np.random.default_rng(20260)
    parts = [np.exp2(rng.uniform(-60.0, 12.0, 17000))]
    pw = np.exp2(np.arange(-60, 13).astype(np.float64))
    dn1, up1 = np.nextafter(pw, 0.0), np.nextafter(pw, np.inf)
    parts += [pw, dn1, up1, np.nextafter(dn1, 0.0), np.nextafter(up1, np.inf)]
    for env in DEMO_ENVS:
        fr = ob.Frirl(env)          # owns the tables `five` borrows
        ve = np.array(fr.five.ve)
        for k in range(ve.shape[0]):
            i, j = rng.integers(0, ve.shape[1], 300), rng.integers(0, ve.shape[1], 300)
            d = ve[k, i] - ve[k, j]
            parts.append((d * d)[d != 0.0])
    parts.append(np.exp2(rng.uniform(-120.0, 120.0, 400)))
    s = np.ascontiguousarray(np.concatenate(parts))
    assert (s > 0).all() and np.isfinite(s).all() and 19000 <= len(s) <= 22000
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def exact():
    """{p: (hi, lo, keep)}: s^(-p/2) = hi + lo for every input, keep = the value is finite and normal in double."""
    s = inputs()
    hi = {p: np.zeros(len(s)) for p in POWERS}
    lo = {p: np.zeros(len(s)) for p in POWERS}
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emax, ctx.Emin = 999999, -999999
        for i, v in enumerate(s.tolist()):
            y = 1 / decimal.Decimal(v).sqrt()
            w = y
            for p in POWERS:
                if p > 1:
                    w = w * y
                h = float(w)
                hi[p][i] = h
                lo[p][i] = float(w - decimal.Decimal(h)) if np.isfinite(h) else 0.0
    tiny = np.finfo(np.float64).tiny
    out = {}
    for p in POWERS:
        keep = np.isfinite(hi[p]) & (hi[p] >= tiny)
        for a in (hi[p], lo[p], keep):
            a.setflags(write=False)
        out[p] = (hi[p], lo[p], keep)
    return out


def rel_error(w, p):
    """max over the kept inputs of |w - s^(-p/2)| / s^(-p/2), and the index where it occurs."""
    hi, lo, keep = exact()[p]
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(((w - hi) - lo) / hi)
    err = np.where(keep, err, 0.0)
    err = np.where(np.isnan(err), np.inf, err)
    i = int(np.argmax(err))
    return float(err[i]), i
