"""Cases of the per-agent hyper-parameter rows (frirl_hip_hparam_rows): which set an agent of a mixed batch learns under, and the
columns that say so to the library.  No GPU needed; tests/test_hparam_rows_ref.py asserts on the oracle alone that the cases are
worth running, tests/test_hip_hparam_rows.py runs them on the device.  The sets, their oracle runs and the point shapes are those of
tests/hparams_cases.py.
"""
import numpy as np

from tests import hparams_cases as hc

# description key -> column of frirl_hip_hparam_rows (frirl_amd.HP_COLUMNS), in hc.HP_KEYS' order
COLUMN = dict(alpha="alpha", gamma="gamma", qdiff_pos="qdiff_pos_boundary", qdiff_neg="qdiff_neg_boundary", weight_thr="weight_significant",
              skip_rules="skip_rules")
assert tuple(COLUMN) == hc.HP_KEYS


def demo_sets(env):
    """The sets of a demo's mixed batch: the demo's own values and every set admitted for whole trajectories on it."""
    return ["default"] + [name for e, name in hc.TRAJ_CASES if e == env]


def columns(descs):
    """Host columns for one description per agent: dict column name -> array [E] (float64; skip_rules int32)."""
    return {COLUMN[k]: np.array([d[k] for d in descs], dtype=np.int32 if k == "skip_rules" else np.float64) for k in hc.HP_KEYS}


# ---- caller-stepped agents on the point shapes: agent e under set (e + ROTATE[shape]) mod 8 of hc.SETS ------------------------------
POINT_SHAPES = [(2, 3)] + hc.EXTERNAL_SHAPES
POINT_E, POINT_EPISODES, POINT_MAXR = 16, 4, 1024
SET_NAMES = list(hc.SETS)
# The rotation per shape at which the oracle alone keeps its near-ties (Mirror.near) within a tenth of the picks: 0 wherever that
# holds (tests/test_hparam_rows_ref.py::test_point_cases_stay_under_the_near_tie_cap asserts it and prints the counts)
ROTATE = {(2, 3): 0, (4, 5): 0, (5, 11): 0, (8, 3): 0}


def point_sets(nant, A):
    return [SET_NAMES[(e + ROTATE[(nant, A)]) % len(SET_NAMES)] for e in range(POINT_E)]


def point_case(nant, A):
    """The shape's base description (the values the Agent carries), environment, start states, and per agent its set's description
    and oracle mirror."""
    from tests.test_hip_external import Mirror, PointEnv, point_desc
    starts = np.ascontiguousarray(np.random.default_rng(nant * 100 + A).uniform(-0.9, 0.9, (POINT_E, nant - 1)))     # new_shape_case's
    descs = [hc.point_desc(nant, A, name) for name in point_sets(nant, A)]
    mirrors = [Mirror(descs[e], starts[e], POINT_MAXR) for e in range(POINT_E)]
    return point_desc(nant, A), PointEnv(nant - 1), starts, descs, mirrors
