"""The references of the population-based-training tests, checked on their own (no GPU, no library): tests/evolve_ref.py::perturb_ref
never leaves [lo, hi], touches CLONED agents and enabled columns only, is a function of (seed, agent, generation, column) alone and
flips exactly where the stream's unit is below the probability; plan_device_ref answers what the device form answers."""
import numpy as np
import pytest

import frirl_amd
from tests.evolve_ref import COLUMNS, DTYPES, PLAN_NAN, PLAN_OK, PLAN_TOO_FEW, perturb_ref, plan_device_ref
from tests.explore_ref import unit
from tests.select_ref import BAD_RULES, BAD_SRC, CHAINED, CLONED, KEPT, plan_ref

E = 64
FULL = dict(alpha=(0.5, 2.0, 0.05, 0.9), gamma=(0.9, 1.1, 0.5, 0.999), weight_significant=(0.25, 4.0, 0.01, 0.5), epsilon=(0.5, 1.5, 0.01, 0.6),
            horizon=(0.5, 2.0, 3, 40), skip_rules=0.5, target=0.3, expected=0.7)


def columns(rng, n=E):
    return dict(alpha=rng.uniform(0.04, 1.0, n), gamma=rng.uniform(0.4, 1.0, n), weight_significant=rng.uniform(0.0, 0.6, n),
                epsilon=rng.uniform(0.0, 0.7, n), horizon=rng.integers(0, 60, n).astype(np.int32), skip_rules=rng.integers(0, 2, n).astype(np.int32),
                target=rng.integers(0, 2, n).astype(np.uint8), expected=rng.integers(0, 2, n).astype(np.uint8))


def statuses(rng, n=E):
    st = rng.choice([KEPT, CLONED, BAD_SRC, CHAINED, BAD_RULES], size=n, p=[0.3, 0.4, 0.1, 0.1, 0.1]).astype(np.int32)
    st[:5] = [KEPT, CLONED, BAD_SRC, CHAINED, BAD_RULES]
    return st


def test_perturbed_values_stay_inside_their_bounds_and_both_clamps_fire():
    rng = np.random.default_rng(1)
    cols, st = columns(rng), statuses(rng)
    spec = frirl_amd.perturb_spec(seed=11, **FULL)
    out = perturb_ref(cols, st, spec, 0)
    cloned = st == CLONED
    for name in COLUMNS[:5]:
        lo, hi = FULL[name][2:]
        assert (out[name][cloned] >= lo).all() and (out[name][cloned] <= hi).all(), name
        assert (out[name][cloned] == lo).any() and (out[name][cloned] == hi).any(), (name, "a clamp never fired")
        assert out[name].dtype == DTYPES[name]
    assert set(np.unique(out["skip_rules"])) <= {0, 1} and set(np.unique(out["target"])) <= {0, 1}


def test_other_agents_and_disabled_columns_stay_bit_for_bit():
    rng = np.random.default_rng(2)
    cols, st = columns(rng), statuses(rng)
    spec = frirl_amd.perturb_spec(seed=5, alpha=FULL["alpha"], horizon=FULL["horizon"], target=1.0)
    out = perturb_ref(cols, st, spec, 3)
    for name in COLUMNS:
        if name in ("alpha", "horizon", "target"):
            assert out[name][st != CLONED].tobytes() == cols[name][st != CLONED].tobytes(), name
            assert (out[name][st == CLONED] != cols[name][st == CLONED]).any(), name
        else:
            assert out[name].tobytes() == cols[name].tobytes(), name
    assert (out["target"][st == CLONED] == 1 - cols["target"][st == CLONED]).all()          # flip 1: everybody
    absent = dict(cols, alpha=None)                                                          # a NULL pointer is skipped
    out = perturb_ref(absent, st, spec, 3)
    assert out["alpha"] is None and (out["horizon"] != cols["horizon"]).any()
    assert all(v is None or v.tobytes() == cols[k].tobytes() for k, v in absent.items()), "the input was modified"


def test_a_draw_depends_on_seed_agent_generation_and_column_alone():
    rng = np.random.default_rng(3)
    cols, st = columns(rng), np.full(E, CLONED, dtype=np.int32)
    spec = frirl_amd.perturb_spec(seed=9, **FULL)
    out = perturb_ref(cols, st, spec, 2)
    again = perturb_ref(cols, st, spec, 2)
    assert all(out[k].tobytes() == again[k].tobytes() for k in COLUMNS)
    # the other agents' values and statuses do not enter: agent e alone in a batch of e + 1 gets the same row
    for e in (0, 7, E - 1):
        alone = {k: v[: e + 1].copy() for k, v in cols.items()}
        for k in alone:
            alone[k][:e] = 0
        one = perturb_ref(alone, np.array([KEPT] * e + [CLONED], dtype=np.int32), spec, 2)
        assert all(one[k][e] == out[k][e] for k in COLUMNS), e
    # the factor is the one the stream's unit picks; another generation or seed picks others
    a = cols["alpha"]
    want = np.array([a[e] * (FULL["alpha"][0] if unit(9, e, 2, 0, 0) < 0.5 else FULL["alpha"][1]) for e in range(E)])
    assert (out["alpha"] == np.clip(want, *FULL["alpha"][2:])).all()
    assert (perturb_ref(cols, st, spec, 3)["alpha"] != out["alpha"]).any()
    assert (perturb_ref(cols, st, frirl_amd.perturb_spec(seed=10, **FULL), 2)["alpha"] != out["alpha"]).any()
    # a column's draw does not depend on which other columns are enabled
    only = perturb_ref(cols, st, frirl_amd.perturb_spec(seed=9, gamma=FULL["gamma"]), 2)
    assert only["gamma"].tobytes() == out["gamma"].tobytes()


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_flags_flip_exactly_where_the_unit_is_below_the_probability(p):
    rng = np.random.default_rng(4)
    cols, st = columns(rng), np.full(E, CLONED, dtype=np.int32)
    spec = frirl_amd.perturb_spec(seed=21, skip_rules=p, target=p, expected=p)
    out = perturb_ref(cols, st, spec, 5)
    for c, name in ((5, "skip_rules"), (6, "target"), (7, "expected")):
        flipped = np.array([unit(21, e, 5, c, 0) < p for e in range(E)])
        assert ((out[name] != cols[name]) == flipped).all(), name
        assert flipped.all() if p == 1.0 else (not flipped.any() if p == 0.0 else 0 < flipped.sum() < E)


def test_horizon_rounds_half_up_and_zero_stays_zero():
    st = np.full(4, CLONED, dtype=np.int32)
    cols = dict(horizon=np.array([0, 1, 3, 1 << 30], dtype=np.int32), epsilon=np.array([0.0, 0.5, 0.0, 1.0]))
    spec = frirl_amd.perturb_spec(seed=1, horizon=(1.5, 1.5, 0, 1 << 30), epsilon=(0.5, 0.5, 0.0, 1.0))
    out = perturb_ref(cols, st, spec, 0)
    assert out["horizon"].tolist() == [0, 2, 5, 1 << 30] and out["epsilon"].tolist() == [0.0, 0.25, 0.0, 0.5]


def test_plan_device_ref_answers_where_the_host_plan_refuses():
    scores = [(2, -1.0), (1, float("nan")), (2, -0.0), (2, 0.0), (0, float("nan"))]
    src, rank, info = plan_device_ref(scores, 1, 1, [1, 0, 1, 1, 0])
    want_src, want_rank = plan_ref(scores, 1, 1, [1, 0, 1, 1, 0])
    assert src.tolist() == want_src.tolist() and rank.tolist() == want_rank.tolist() + [-1, -1] and info == (3, PLAN_OK, 2, -1)
    src, rank, info = plan_device_ref(scores, 1, 1, [1, 0, 1, 1, 1])
    assert src.tolist() == list(range(5)) and rank.tolist() == [-1] * 5 and info == (4, PLAN_NAN, -1, 4)
    assert plan_device_ref(scores, 1, 1)[2] == (5, PLAN_NAN, -1, 1)
    src, rank, info = plan_device_ref(scores, 2, 2, [1, 0, 1, 1, 0])
    assert src.tolist() == list(range(5)) and rank.tolist() == [-1] * 5 and info == (3, PLAN_TOO_FEW, -1, -1)
    assert plan_device_ref(scores, 1, 1, [0] * 5)[2] == (0, PLAN_TOO_FEW, -1, -1)
    for bad in ((0, 1), (1, -1), (3, 3)):
        with pytest.raises(ValueError):
            plan_device_ref(scores, *bad)
