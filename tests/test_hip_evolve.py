"""Population-based training on the device (csrc/select_device.hip and the frirl_hip_batch_evolve* calls of csrc/batch.hip).

1. frirl_hip_select_plan_device against tests/evolve_ref.py::plan_device_ref (tests/select_ref.py::plan_ref with the device's answers
   where the host form refuses), exact, every output between sentinels
2. frirl_hip_perturb_rows against tests/evolve_ref.py::perturb_ref, bit for bit
3. frirl_hip_batch_evolve_step(spec = NULL) equals frirl_hip_batch_select on a twin batch; with a spec the rows are perturb_ref of the
   inherited rows; refusals leave the batch as it was; frirl_hip_batch_evolve is the loop of train + step; frirl_demo

The batch object is opaque: its state is read through the getters, and what those do not show through the episodes trained afterwards.
Everything here is exact: the plan is integers, the perturbation one rounded multiplication per value."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frirl_amd
from tests import hparam_rows_cases as rc
from tests import hparams_cases as hc
from tests.evolve_ref import COLUMNS, PLAN_NAN, PLAN_OK, PLAN_TOO_FEW, perturb_ref, plan_device_ref
from tests.select_ref import BAD_RULES, BAD_SRC, CHAINED, CLONED, KEPT, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCORE = np.dtype([("rows", "<i4"), ("successes", "<i4"), ("steps_sum", "<i8"), ("reward_sum", "<f8"), ("reward_min", "<f8"), ("reward_max", "<f8")])
PAD = 16                    # sentinel int32s on either side of src and rank
SENTINEL = -777


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------
def run_plan(pairs, parents, replace, eligible=None):
    """frirl_hip_select_plan_device on (successes, reward_sum) pairs: (src, rank, info) as host lists, the outputs inside sentinels."""
    import torch
    E = len(pairs)
    host = np.zeros(E, dtype=SCORE)
    host["successes"], host["reward_sum"] = [p[0] for p in pairs], [p[1] for p in pairs]
    host["rows"], host["reward_min"], host["reward_max"] = 3, np.nan, np.nan              # fields the plan must not read
    scores = torch.from_numpy(host.view(np.uint8).reshape(E, SCORE.itemsize).copy()).to(DEV)
    el = None if eligible is None else torch.tensor(np.asarray(eligible, dtype=np.uint8)).to(DEV)
    out = torch.full((2, E + 2 * PAD), SENTINEL, dtype=torch.int32, device=DEV)
    info = torch.full((4 + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    frirl_amd.check(frirl_amd.lib().frirl_hip_select_plan_device(scores.data_ptr(), E, None if el is None else el.data_ptr(), parents, replace,
                                                                  out[0, PAD:].data_ptr(), out[1, PAD:].data_ptr(), info[PAD:].data_ptr(), None),
                    "frirl_hip_select_plan_device")
    torch.cuda.synchronize()
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert (out[:, :PAD] == SENTINEL).all() and (out[:, PAD + E:] == SENTINEL).all() and (info[:PAD] == SENTINEL).all() and (info[PAD + 4:] == SENTINEL).all()
    return out[0, PAD: PAD + E].tolist(), out[1, PAD: PAD + E].tolist(), tuple(info[PAD: PAD + 4].tolist())


def check_plan(pairs, parents, replace, eligible=None):
    src, rank, info = run_plan(pairs, parents, replace, eligible)
    want_src, want_rank, want_info = plan_device_ref(pairs, parents, replace, eligible)
    where = (len(pairs), parents, replace, None if eligible is None else int(np.sum(eligible)))
    assert info == want_info, (where, info, want_info)
    assert rank == want_rank.tolist(), (where, np.argwhere(np.array(rank) != want_rank)[:4].tolist())
    assert src == want_src.tolist(), (where, np.argwhere(np.array(src) != want_src)[:4].tolist())
    return src, rank, info


def tied_pairs(E, rng):
    return list(zip(rng.integers(0, 4, E).tolist(), rng.choice([-np.inf, -7.5, -0.0, 0.0, 3.25], E).tolist()))


def test_plan_of_one_agent_and_of_equal_scores():
    assert check_plan([(1, -3.0)], 1, 0) == ([0], [0], (1, PLAN_OK, 0, -1))
    src, rank, info = check_plan([(2, -5.0)] * 7, 2, 3)
    assert rank == list(range(7)) and src == [0, 1, 2, 3, 0, 1, 0] and info == (7, PLAN_OK, 0, -1)
    _, rank, _ = check_plan([(2, -0.0), (2, 0.0)] * 3 + [(2, 0.0)], 1, 6)                 # -0.0 ties with +0.0: the index decides
    assert rank == list(range(7))


@pytest.mark.parametrize("E", [257, 300, 5000])
def test_plan_matches_the_reference_on_heavily_tied_scores(E):
    """257 and 300: across one tile of 256 keys and several workgroups of 64 agents, no multiple of 64; 5000: twenty tiles.  Successes
    from 0..3 and rewards from {-inf, -7.5, -0.0, 0.0, 3.25}: most comparisons are decided by the index."""
    rng = np.random.default_rng(E)
    pairs = tied_pairs(E, rng)
    check_plan(pairs, E // 4, E // 2)
    check_plan(pairs, 1, E - 1)                                                           # one parent fans out to everybody
    check_plan(pairs, E, 0)                                                               # nothing replaced, everybody ranked
    check_plan(pairs, 3, 0)
    mask = (rng.random(E) < 0.6).astype(np.uint8)
    N = int(mask.sum())
    check_plan(pairs, 5, N // 3, mask)
    src, rank, info = check_plan(pairs, N - 7, 7, mask)                                   # N == parents + replace exactly
    assert info[:2] == (N, PLAN_OK) and rank[N:] == [-1] * (E - N) and sorted(rank[:N]) == np.nonzero(mask)[0].tolist()
    one = np.zeros(E, dtype=np.uint8)
    one[E - 2] = 1
    assert check_plan(pairs, 1, 0, one)[1][:2] == [E - 2, -1]
    assert check_plan(pairs, 1, 0, np.zeros(E, dtype=np.uint8))[2] == (0, PLAN_TOO_FEW, -1, -1)      # N == 0


def test_plan_orders_distinct_rewards_of_any_size():
    rng = np.random.default_rng(77)
    pairs = [(1, float(r)) for r in np.concatenate([rng.normal(size=120) * 10.0 ** rng.integers(-300, 300, 120), [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324]])]
    check_plan(pairs, 10, 50)


def test_plan_refusals_decided_on_the_device():
    rng = np.random.default_rng(9)
    E = 300
    pairs = tied_pairs(E, rng)
    pairs[100], pairs[37], pairs[299] = (5, float("nan")), (0, float("nan")), (1, float("nan"))
    mask = np.ones(E, dtype=np.uint8)
    mask[[37, 100, 299]] = 0
    src, rank, info = check_plan(pairs, 4, 20, mask)                                      # a NaN of an agent that takes no part is ignored
    assert info[:2] == (E - 3, PLAN_OK) and not {37, 100, 299} & set(rank)
    mask[[100, 299]] = 1
    src, rank, info = check_plan(pairs, 4, 20, mask)
    assert info == (E - 1, PLAN_NAN, -1, 100) and src == list(range(E)) and rank == [-1] * E
    assert check_plan(pairs, 4, 20)[2] == (E, PLAN_NAN, -1, 37)                           # the lowest index, not the first workgroup to finish
    few = np.zeros(E, dtype=np.uint8)
    few[:23] = 1
    src, rank, info = check_plan(pairs, 4, 20, few)                                       # 24 > 23 eligible
    assert info == (23, PLAN_TOO_FEW, -1, -1) and src == list(range(E)) and rank == [-1] * E
    assert check_plan(pairs, 3, 20, few)[2][:2] == (23, PLAN_OK)


def test_problem_select_plan_device_returns_tensors():
    import torch
    E = 9
    host = np.zeros(E, dtype=SCORE)
    host["successes"], host["reward_sum"] = np.arange(E) % 3, -np.arange(E, dtype=np.float64)
    scores = torch.from_numpy(host.view(np.uint8).reshape(E, SCORE.itemsize).copy()).to(DEV)
    src, rank, info = frirl_amd.select_plan_device(scores, 2, 3, eligible=torch.ones(E, dtype=torch.bool, device=DEV))
    want_src, want_rank = plan_ref(list(zip(host["successes"].tolist(), host["reward_sum"].tolist())), 2, 3)
    assert src.tolist() == want_src.tolist() and rank.tolist() == want_rank.tolist() and info.tolist() == [E, PLAN_OK, int(want_rank[0]), -1]
    with pytest.raises(frirl_amd.FrirlHipError, match="parents=5"):
        frirl_amd.select_plan_device(scores, 5, 5)


# ---- 2. the perturbation -------------------------------------------------------------------------------------------------------------
EP = 300
FULL = dict(alpha=(0.5, 2.0, 0.05, 0.9), gamma=(0.9, 1.1, 0.5, 0.999), weight_significant=(0.25, 4.0, 0.01, 0.5), epsilon=(0.5, 1.5, 0.01, 0.6),
            horizon=(0.5, 2.0, 1, 1 << 30), skip_rules=0.5, target=0.5, expected=0.5)


def perturb_inputs(rng, E=EP):
    cols = dict(alpha=rng.uniform(0.04, 1.0, E), gamma=rng.uniform(0.4, 1.0, E), weight_significant=rng.uniform(0.0, 0.6, E), epsilon=rng.uniform(0.0, 0.7, E),
                horizon=rng.integers(0, 60, E).astype(np.int32), skip_rules=rng.integers(0, 2, E).astype(np.int32),
                target=rng.integers(0, 2, E).astype(np.uint8), expected=rng.integers(0, 2, E).astype(np.uint8),
                qdiff_pos_boundary=rng.uniform(1.0, 2.0, E), qdiff_neg_boundary=rng.uniform(-2.0, -1.0, E))
    cols["horizon"][:6] = [0, 1, 1 << 30, 0, 1, 1 << 30]
    cols["epsilon"][:3] = [0.0, 0.0, 1.0]
    status = rng.choice([KEPT, CLONED, BAD_SRC, CHAINED, BAD_RULES], size=E, p=[0.25, 0.45, 0.1, 0.1, 0.1]).astype(np.int32)
    status[:10] = [CLONED, CLONED, CLONED, KEPT, BAD_SRC, CHAINED, BAD_RULES, CLONED, KEPT, CLONED]
    return cols, status


def run_perturb(cols, status, spec, generation, absent=()):
    """frirl_hip_perturb_rows on device copies of the columns (those in `absent` are NULL pointers): (columns afterwards, count)."""
    import torch
    E = len(status)
    have = {k: (None if k in absent else v) for k, v in cols.items()}
    rows = frirl_amd.HparamRows(E, DEV, **{k: have[k] for k in frirl_amd.HP_COLUMNS})
    explore = frirl_amd.ExploreRows(E, DEV, epsilon=have["epsilon"], horizon=have["horizon"])
    target = frirl_amd.TargetRows(E, DEV, target=have["target"])
    expect = frirl_amd.ExpectRows(E, DEV, expected=have["expected"])
    st = torch.from_numpy(status).to(DEV)
    count = frirl_amd.perturb_rows(spec, generation, st, rows=rows, explore=explore, target=target, expect=expect)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tobytes() == status.tobytes()
    owner = dict(epsilon=explore, horizon=explore, target=target, expected=expect)
    after = {k: (None if have[k] is None else getattr(owner.get(k, rows), k).cpu().numpy()) for k in cols}
    return after, int(count.item())


def assert_columns_equal(got, want, where):
    for k, v in want.items():
        assert (got[k] is None) == (v is None), (where, k)
        if v is not None:
            assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), (where, k, np.argwhere(got[k] != v)[:4].tolist())


@pytest.mark.parametrize("flip", [0.0, 0.5, 1.0])
def test_perturb_rows_matches_the_reference_bit_for_bit(flip):
    """300 agents (two workgroups, no multiple of 64) of all five CLONE_* statuses, every column enabled; horizons 0, 1 and 2^30; steps
    and bounds under which both clamps fire; the qdiff columns, which no spec can name, are beside them and stay."""
    cols, status = perturb_inputs(np.random.default_rng(12))
    spec = frirl_amd.perturb_spec(seed=0x1234567890ABCDEF, **dict(FULL, skip_rules=flip, target=flip, expected=flip))
    want = perturb_ref(cols, status, spec, 4)
    got, count = run_perturb(cols, status, spec, 4)
    assert_columns_equal(got, want, flip)
    cloned = status == CLONED
    assert count == int(cloned.sum())
    for name in COLUMNS[:4]:
        lo, hi = FULL[name][2:]
        assert (got[name][cloned] == lo).any() and (got[name][cloned] == hi).any(), (name, "a clamp never fired")
    assert got["horizon"][0] == 1 and got["horizon"][1] in (1, 2) and got["horizon"][2] in (1 << 29, 1 << 30) and got["epsilon"][0] == 0.01
    assert (got["horizon"][[2, 5]] == 1 << 30).any(), "2^30 * 2 was never clamped"
    for name in COLUMNS[5:]:
        changed = got[name][cloned] != cols[name][cloned]
        assert changed.all() if flip == 1.0 else (not changed.any() if flip == 0.0 else 0 < changed.sum() < cloned.sum()), name
    for name in cols:
        assert got[name][~cloned].tobytes() == cols[name][~cloned].tobytes(), name


@pytest.mark.parametrize("absent,enabled", [(("alpha", "horizon", "target"), COLUMNS), ((), ("gamma", "horizon", "expected")),
                                            (("gamma", "weight_significant", "skip_rules", "qdiff_pos_boundary", "qdiff_neg_boundary", "alpha"), COLUMNS),
                                            (COLUMNS, COLUMNS)], ids=["some-null", "some-disabled", "no-hparams", "all-null"])
def test_perturb_rows_skips_null_and_disabled_columns(absent, enabled):
    cols, status = perturb_inputs(np.random.default_rng(13))
    spec = frirl_amd.perturb_spec(seed=3, **{k: FULL[k] for k in enabled})
    want = perturb_ref({k: (None if k in absent else v) for k, v in cols.items()}, status, spec, 0)
    got, count = run_perturb(cols, status, spec, 0, absent=absent)
    assert_columns_equal(got, want, (absent, enabled))
    assert count == (0 if set(absent) >= set(COLUMNS) else int((status == CLONED).sum()))
    for k in cols:
        if k not in enabled and k not in absent:
            assert got[k].tobytes() == cols[k].tobytes(), k


def test_perturb_draws_change_with_the_generation_and_repeat_within_it():
    cols, status = perturb_inputs(np.random.default_rng(14))
    spec = frirl_amd.perturb_spec(seed=8, **FULL)
    a, _ = run_perturb(cols, status, spec, 0)
    b, _ = run_perturb(cols, status, spec, 0)
    c, _ = run_perturb(cols, status, spec, 1)
    assert_columns_equal(a, b, "the same generation twice")
    assert_columns_equal(c, perturb_ref(cols, status, spec, 1), "generation 1")
    assert all((a[k] != c[k]).any() for k in COLUMNS)


# ---- 3. the batch object -------------------------------------------------------------------------------------------------------------
def train(batch, max_episodes):
    ran = C.c_int32(0)
    frirl_amd.check(frirl_amd.lib().frirl_hip_batch_train(batch, max_episodes, C.byref(ran)), "frirl_hip_batch_train")
    return ran.value


def rulebase(batch, e, nant):
    R = C.c_int32(0)
    lib = frirl_amd.lib()
    frirl_amd.check(lib.frirl_hip_batch_get_rulebase(batch, e, C.byref(R), None, None), "frirl_hip_batch_get_rulebase")
    rant, rconc = np.zeros((R.value, nant)), np.zeros(R.value)
    frirl_amd.check(lib.frirl_hip_batch_get_rulebase(batch, e, C.byref(R), rant.ctypes.data_as(frirl_amd._DP), rconc.ctypes.data_as(frirl_amd._DP)), "frirl_hip_batch_get_rulebase")
    return rant, rconc


def batch_rows(batch):
    """The rows every agent trains under, by the names of tests/evolve_ref.py::COLUMNS (and the two qdiff columns)."""
    out = dict(frirl_amd.batch_get_hparams(batch))
    out.update(frirl_amd.batch_get_exploration(batch))
    out["target"], out["expected"] = frirl_amd.batch_get_target(batch), frirl_amd.batch_get_expected(batch)
    return out


def batch_state(batch, E, nant):
    """Everything the getters show, as bytes per key."""
    out = {k: v.tobytes() for k, v in frirl_amd.batch_agent_report(batch).items()}
    out.update({"row_" + k: v.tobytes() for k, v in batch_rows(batch).items()})
    for e in range(E):
        rant, rconc = rulebase(batch, e, nant)
        out[f"rant{e}"], out[f"rconc{e}"] = rant.tobytes(), rconc.tobytes()
    return out


def select_batch(E, all_rows=False):
    """Mountaincar agents that differ in start state and hyper-parameter set, 12 episodes in (the recipe of tests/test_hip_select.py);
    all_rows: every agent also has an exploration row, a TD target and an expected-SARSA flag of its own."""
    env = "mountaincar"
    d = frirl_amd.demo_describe(env)
    rng = np.random.default_rng(4)
    start = np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1)
    sets = rc.demo_sets(env)
    batch = frirl_amd.demo_batch_object(env, E, 512, start_states=start, seed=17)
    frirl_amd.batch_set_hparams(batch, **rc.columns([hc.demo_desc(env, sets[e % len(sets)]) for e in range(E)]))
    if all_rows:
        frirl_amd.batch_set_exploration(batch, epsilon=np.linspace(0.2, 0.5, E), horizon=np.arange(E, dtype=np.int32) % 3 * 40)
        frirl_amd.batch_set_target(batch, target=np.arange(E, dtype=np.uint8) % 2)
        frirl_amd.batch_set_expected(batch, expected=np.arange(E, dtype=np.uint8) // 2 % 2)
    train(batch, 13)
    return batch, d


def eval_starts(d, E, n):
    rng = np.random.default_rng(8)
    return np.stack([rng.choice(d["grids"][k], (E, n)) for k in range(d["nstates"])], 2)


def test_evolve_step_without_a_spec_is_batch_select():
    E, n, parents, replace = 8, 2, 2, 3
    lib = frirl_amd.lib()
    one, d = select_batch(E)
    two, _ = select_batch(E)
    nant = d["nant"]
    try:
        starts = eval_starts(d, E, n)
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        before = batch_state(one, E, nant)
        res = frirl_amd.batch_evolve_step(one, n, parents, replace, start_states=starts)
        scores, src, want = frirl_amd.batch_select(two, n, parents, replace, start_states=starts)
        after = batch_state(one, E, nant)
        assert after == batch_state(two, E, nant)
        assert after != before, "the selection replaced nothing that can be seen"
        assert (res.best, res.parents, res.replaced, res.rules_copied) == (want.best, want.parents, want.replaced, want.rules_copied)
        assert (res.replaced, res.perturbed, res.generation, res.plan_status) == (replace, 0, 0, PLAN_OK)
        succ, reward = C.c_int32(-1), C.c_double(0.0)
        frirl_amd.check(lib.frirl_hip_batch_evolve_best_score(one, C.byref(succ), C.byref(reward)), "frirl_hip_batch_evolve_best_score")
        assert (succ.value, reward.value) == (scores[want.best].successes, scores[want.best].reward_sum)
        train(one, 4), train(two, 4)        # the sticky flag, the index mirror and the spread state are read by these episodes
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        assert frirl_amd.batch_evolve_step(one, n, parents, replace, start_states=starts, inherit_rows=True).generation == 1
        frirl_amd.batch_select(two, n, parents, replace, start_states=starts, inherit_rows=True)
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
    finally:
        lib.frirl_hip_batch_destroy(one)
        lib.frirl_hip_batch_destroy(two)


def test_evolve_step_perturbs_the_inherited_rows():
    """Every row set on the batch, inherit_rows = 1 and a spec over all eight columns: the rows afterwards are perturb_ref of the rows
    frirl_hip_batch_select(inherit_rows = 1) leaves on a twin, everything else is the twin's; the second step draws under generation 1."""
    E, n, parents, replace = 8, 2, 2, 3
    lib = frirl_amd.lib()
    one, d = select_batch(E, all_rows=True)
    two, _ = select_batch(E, all_rows=True)
    nant = d["nant"]
    spec = frirl_amd.perturb_spec(seed=99, alpha=(0.8, 1.25, 0.05, 1.0), gamma=(0.95, 1.02, 0.5, 0.9999), weight_significant=(0.5, 2.0, 0.0, 0.4),
                                  epsilon=(0.5, 1.5, 0.0, 0.5), horizon=(1.0, 2.0, 0, 200), skip_rules=0.5, target=0.5, expected=0.5)
    try:
        starts = eval_starts(d, E, n)
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        for generation in (0, 1):
            res = frirl_amd.batch_evolve_step(one, n, parents, replace, start_states=starts, inherit_rows=True, spec=spec)
            _, src, want = frirl_amd.batch_select(two, n, parents, replace, start_states=starts, inherit_rows=True)
            status = np.where(src != np.arange(E), CLONED, KEPT).astype(np.int32)
            inherited = batch_rows(two)
            expect = perturb_ref(inherited, status, spec, generation)
            got = batch_rows(one)
            assert_columns_equal(got, expect, generation)
            assert any(got[k].tobytes() != inherited[k].tobytes() for k in COLUMNS), "nothing was perturbed"
            assert (res.best, res.replaced, res.rules_copied) == (want.best, want.replaced, want.rules_copied)
            assert (res.perturbed, res.replaced, res.generation, res.plan_status) == (replace, replace, generation, PLAN_OK)
            a, b = batch_state(one, E, nant), batch_state(two, E, nant)
            assert {k: v for k, v in a.items() if not k.startswith("row_")} == {k: v for k, v in b.items() if not k.startswith("row_")}
            # the twin goes on under the same rows: put them there the way a host-side loop would have to
            frirl_amd.batch_set_hparams(two, **{k: got[k] for k in frirl_amd.HP_COLUMNS})
            frirl_amd.batch_set_exploration(two, epsilon=got["epsilon"], horizon=got["horizon"])
            frirl_amd.batch_set_target(two, target=got["target"])
            frirl_amd.batch_set_expected(two, expected=got["expected"])
            report = frirl_amd.batch_agent_report(one)
            learning = report["converged"] == 0
            assert learning[status == CLONED].all(), report["converged"]                 # a clone's convergence state is cleared
            train(one, 4), train(two, 4)
            assert batch_state(one, E, nant) == batch_state(two, E, nant)
            # training goes on: three more episodes for everybody who had not met the stopping rule, fewer only for an agent that meets
            # it on the way; an agent that had met it sits out, as ever
            later = frirl_amd.batch_agent_report(one)
            more = later["episodes"] - report["episodes"]
            assert (more[~learning] == 0).all() and ((more == 3) | ((later["converged"] == 1) & (more >= 1)))[learning].all(), (report, later)
            assert (more[status == CLONED] >= 1).all()
    finally:
        lib.frirl_hip_batch_destroy(one)
        lib.frirl_hip_batch_destroy(two)


def test_refused_evolve_steps_leave_the_batch_as_it_was():
    E = 5
    lib = frirl_amd.lib()
    batch, d = select_batch(E)
    nant = d["nant"]
    alpha = (0.8, 1.25, 0.05, 1.0)
    try:
        before = batch_state(batch, E, nant)
        for kw, word in ((dict(n=1, parents=1, replace=1, spec=frirl_amd.perturb_spec(epsilon=(0.5, 2.0, 0.0, 1.0))), "epsilon"),
                         (dict(n=1, parents=1, replace=1, spec=frirl_amd.perturb_spec(alpha=alpha, target=0.5)), "target"),
                         (dict(n=1, parents=1, replace=1, spec=frirl_amd.perturb_spec(alpha=(0.8, 17.0, 0.05, 1.0))), "alpha: up"),
                         (dict(n=1, parents=3, replace=3), "parents=3"), (dict(n=1, parents=0, replace=1), "parents=0"),
                         (dict(n=1, parents=1, replace=-1), "replace=-1"), (dict(n=0, parents=1, replace=1), "n=0")):
            with pytest.raises(frirl_amd.FrirlHipError, match="frirl_hip_batch_evolve_step: .*" + word):
                frirl_amd.batch_evolve_step(batch, **kw)
        with pytest.raises(frirl_amd.FrirlHipError, match="frirl_hip_batch_evolve: .*gamma"):
            frirl_amd.batch_evolve(batch, 2, 4, 1, 1, 1, spec=frirl_amd.perturb_spec(gamma=(0.5, 32.0, 0.0, 1.0)))
        with pytest.raises(frirl_amd.FrirlHipError, match="generations=0"):
            frirl_amd.batch_evolve(batch, 0, 4, 1, 1, 1)
        assert lib.frirl_hip_batch_evolve_best_score(batch, None, None) == -2
        assert batch_state(batch, E, nant) == before
        res = frirl_amd.batch_evolve_step(batch, 1, 1, 1, spec=frirl_amd.perturb_spec(alpha=alpha))
        assert res.generation == 0, "a refused step advanced the generation counter"
        twin, _ = select_batch(E)
        try:
            frirl_amd.batch_evolve_step(twin, 1, 1, 1, spec=frirl_amd.perturb_spec(alpha=alpha))
            train(batch, 3), train(twin, 3)
            assert batch_state(batch, E, nant) == batch_state(twin, E, nant), "a refused call left something behind that training read"
        finally:
            lib.frirl_hip_batch_destroy(twin)
    finally:
        lib.frirl_hip_batch_destroy(batch)


def test_batch_evolve_is_the_loop_of_train_and_step():
    E, n, parents, replace = 8, 1, 2, 3
    lib = frirl_amd.lib()
    one, d = select_batch(E)
    two, _ = select_batch(E)
    nant = d["nant"]
    spec = frirl_amd.perturb_spec(seed=5, alpha=(0.8, 1.25, 0.05, 1.0), skip_rules=0.5)
    try:
        results = frirl_amd.batch_evolve(one, 2, 4, n, parents, replace, inherit_rows=True, spec=spec)          # the agents' own start states
        by_hand = []
        for g in range(2):
            assert train(two, 5) == 4
            by_hand.append(frirl_amd.batch_evolve_step(two, n, parents, replace, inherit_rows=True, spec=spec))
        fields = [k for k, _ in frirl_amd.EvolveResult._fields_]
        assert [[getattr(r, k) for k in fields] for r in results] == [[getattr(r, k) for k in fields] for r in by_hand]
        assert [r.generation for r in results] == [0, 1] and all(r.perturbed == replace for r in results)
        assert batch_state(one, E, nant) == batch_state(two, E, nant)
        assert frirl_amd.batch_agent_report(one)["episodes"].max() == 12 + 8
    finally:
        lib.frirl_hip_batch_destroy(one)
        lib.frirl_hip_batch_destroy(two)


# ---- the demo ------------------------------------------------------------------------------------------------------------------------
DEMO = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
LINE = r"select {env}: generation (\d+) best (\d+) successes (\d+) reward (-?[\d.]+) replaced (\d+) rules_copied (\d+)"


def run_demo(tmp_path, extra):
    env = "mountaincar"
    sets = rc.demo_sets(env)
    f = tmp_path / "f.txt"
    f.write_text("".join(" ".join(repr(float(hc.demo_desc(env, n)[k])) for k in hc.HP_KEYS) + "\n" for n in sets))
    return subprocess.run([DEMO, "--env", env, "--agents", "8", "--hparams", str(f), "--select-episodes", "4", "--select-parents", "2", "--select-replace", "3",
                           "--select-inherit", "--evaluate", "2", "--max-episodes", "12"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_demo_perturbs_the_clones_rows(tmp_path):
    env = "mountaincar"
    r = run_demo(tmp_path, ["--select", "2", "--select-perturb", "alpha:0.8:1.25:0.05:1.0", "--select-seed", "3"])
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(f"select {env}: ")]
    assert len(lines) == 2, r.stdout
    for g, line in enumerate(lines):
        m = re.match(LINE.format(env=env) + r" perturbed (\d+)$", line)
        assert m, line
        assert int(m[1]) == g and 0 <= int(m[2]) < 8 and 0 <= int(m[3]) <= 2 and int(m[5]) == 3 and int(m[6]) >= 3 * 2 ** 3 and int(m[7]) == 3
    plain = run_demo(tmp_path, ["--select", "2"])
    assert plain.returncode == 0, plain.stderr
    old = [l for l in plain.stdout.splitlines() if l.startswith(f"select {env}: ")]
    assert len(old) == 2 and all(re.match(LINE.format(env=env) + "$", l) for l in old), plain.stdout
    assert old[0] + " perturbed 3" == lines[0], "generation 0 selects before anything was perturbed: the same line but for its new end"
    for out in (r.stdout, plain.stdout):
        report = [l for l in out.splitlines() if l.startswith(f"batch {env}: agents 8 episodes ")]
        assert len(report) == 1 and int(report[0].split()[5]) == 11, out


def test_demo_refuses_perturbation_without_selection(tmp_path):
    r = run_demo(tmp_path, ["--select-perturb", "alpha:0.8:1.25:0.05:1.0"])
    assert r.returncode == 2 and "go with --select G" in r.stderr, r.stderr
