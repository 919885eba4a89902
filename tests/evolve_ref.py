"""numpy / plain-Python restatements of the population-based-training contract of include/frirl_hip.h (frirl_hip_select_plan_device,
frirl_hip_perturb_rows), written from the contract, not from the kernels.  No GPU needed.

The ranking itself is tests/select_ref.py::plan_ref; plan_device_ref adds what the device form answers instead of refusing."""
import math

import numpy as np

from tests.explore_ref import unit
from tests.select_ref import CLONED, plan_ref

COLUMNS = ("alpha", "gamma", "weight_significant", "epsilon", "horizon", "skip_rules", "target", "expected")      # FRIRL_HIP_PERTURB_*
DTYPES = dict(alpha=np.float64, gamma=np.float64, weight_significant=np.float64, epsilon=np.float64, horizon=np.int32, skip_rules=np.int32,
              target=np.uint8, expected=np.uint8)
PLAN_OK, PLAN_NAN, PLAN_TOO_FEW = range(3)


def plan_device_ref(scores, parents, replace, eligible=None):
    """scores: sequence of (successes, reward_sum).  Returns (src [E], rank [E] padded with -1, (N, status, best, bad_agent)) of
    frirl_hip_select_plan_device; ValueError for what the host already refuses (sizes, parents + replace > E)."""
    E = len(scores)
    if E < 1 or parents < 1 or replace < 0 or parents + replace > E:
        raise ValueError("sizes")
    who = [e for e in range(E) if eligible is None or eligible[e]]
    identity, nobody = np.arange(E, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    nan = [e for e in who if scores[e][1] != scores[e][1]]
    if nan:
        return identity, nobody, (len(who), PLAN_NAN, -1, nan[0])
    if parents + replace > len(who):
        return identity, nobody, (len(who), PLAN_TOO_FEW, -1, -1)
    src, rank = plan_ref(scores, parents, replace, eligible)
    padded = nobody.copy()
    padded[: len(rank)] = rank
    return src, padded, (len(who), PLAN_OK, int(rank[0]), -1)


def perturb_ref(columns, status, spec, generation):
    """columns: dict name -> numpy array [E] or None (a NULL pointer), names as COLUMNS; status [E] of CLONE_*; spec: anything with the
    fields of frirl_hip_perturb_spec (columns, seed, down, up, lo, hi, flip).  Returns the dict after frirl_hip_perturb_rows; the
    input is not modified."""
    out = {k: (None if v is None else np.array(v, copy=True)) for k, v in columns.items()}
    for e in np.nonzero(np.asarray(status) == CLONED)[0].tolist():
        for c, name in enumerate(COLUMNS):
            col = out.get(name)
            if col is None or not (int(spec.columns) >> c) & 1:
                continue
            u = unit(int(spec.seed), e, int(generation), c, 0)
            if c >= 5:
                if u < spec.flip[c - 5]:
                    col[e] = 1 - int(col[e])
                continue
            f = float(spec.down[c]) if u < 0.5 else float(spec.up[c])
            lo, hi = float(spec.lo[c]), float(spec.hi[c])
            if c < 4:
                col[e] = np.fmin(np.fmax(np.float64(col[e]) * np.float64(f), lo), hi)      # one rounded multiplication
            else:
                x = math.floor(float(col[e]) * f + 0.5)
                col[e] = int(np.fmin(np.fmax(float(x), lo), hi))
    return out
