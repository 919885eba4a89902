"""Host side of the selection calls (no GPU needed): frirl_hip_select_plan against tests/select_ref.py::plan_ref, its refusals, the
argument checks frirl_hip_clone_agents makes before it looks for a device, and the new ABI symbols."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from tests.select_ref import plan_ref

NEW = ("frirl_hip_clone_agents", "frirl_hip_select_plan", "frirl_hip_batch_clone", "frirl_hip_batch_select", "frirl_hip_batch_get_hparams",
       "frirl_hip_batch_get_exploration")
EINVAL = -2
I32 = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    for fn in ("select_plan", "batch_clone", "batch_select", "batch_get_hparams", "batch_get_exploration"):
        assert callable(getattr(frirl_amd, fn)), fn
    assert callable(frirl_amd.Problem.clone_agents)
    assert C.sizeof(frirl_amd.SelectResult) == 24 and frirl_amd.SelectResult.rules_copied.offset == 16
    assert (frirl_amd.CLONE_KEPT, frirl_amd.CLONE_CLONED, frirl_amd.CLONE_BAD_SRC, frirl_amd.CLONE_CHAINED, frirl_amd.CLONE_BAD_RULES) == (0, 1, 2, 3, 4)


def both(scores, parents, replace, eligible=None):
    src, rank = frirl_amd.select_plan(scores, parents, replace, eligible)
    rsrc, rrank = plan_ref(scores, parents, replace, eligible)
    assert src.tolist() == rsrc.tolist() and rank.tolist() == rrank.tolist(), (scores, parents, replace, eligible)
    return src.tolist(), rank.tolist()


def test_ties_in_successes_go_to_the_reward(lib):
    scores = [(2, -300.0), (3, -500.0), (2, -100.0), (3, -400.0), (0, 0.0), (2, -200.0)]
    src, rank = both(scores, 2, 2)
    assert rank == [3, 1, 2, 5, 0, 4] and src == [1, 1, 2, 3, 3, 5]


def test_ties_in_both_keys_go_to_the_lower_index(lib):
    scores = [(1, -5.0)] * 3 + [(2, -5.0)] * 2 + [(1, -5.0)]
    src, rank = both(scores, 1, 3)
    assert rank == [3, 4, 0, 1, 2, 5] and src == [0, 3, 3, 3, 4, 3]


def test_an_eligible_mask_restricts_rank_and_replacement(lib):
    scores = [(5, 0.0), (0, -9.0), (4, 0.0), (1, 0.0), (0, -1.0), (3, 0.0)]
    eligible = [0, 1, 1, 1, 0, 1]
    src, rank = both(scores, 1, 2, eligible)
    assert rank == [2, 5, 3, 1] and src == [0, 2, 2, 2, 4, 5]      # agent 0, the best of all, and agent 4 take no part


def test_replace_zero_is_the_identity(lib):
    src, rank = both([(0, -1.0), (1, -1.0), (1, 0.0)], 2, 0)
    assert src == [0, 1, 2] and rank == [2, 1, 0]


def test_one_parent_fans_out(lib):
    src, _ = both([(e % 3, -float(e)) for e in range(9)], 1, 8)
    assert src == [2] * 9


def test_parents_plus_replace_may_equal_the_eligible_agents_exactly(lib):
    scores = [(e, 0.0) for e in range(7)]
    src, _ = both(scores, 3, 4)
    assert src == [6, 5, 4, 6, 4, 5, 6]
    both(scores, 3, 2, [1, 1, 0, 1, 1, 0, 1])
    both([(1, 1.0)], 1, 0)


def test_reward_keys_of_any_size_order_as_doubles(lib):
    both([(1, float("inf")), (1, -float("inf")), (1, 0.0), (1, -0.0), (1, 1e300), (1, -1e-300)], 2, 3)


def test_no_parent_is_replaced_on_random_tables(lib):
    rng = np.random.default_rng(23)
    for _ in range(300):
        E = int(rng.integers(1, 40))
        scores = [(int(rng.integers(0, 4)), float(rng.choice([-100.0, -50.0, 0.0, rng.normal()]))) for _ in range(E)]
        eligible = None if rng.random() < 0.5 else (rng.random(E) < 0.7).astype(np.uint8)
        if eligible is not None and eligible.sum() == 0:
            eligible[int(rng.integers(E))] = 1
        N = E if eligible is None else int(eligible.sum())
        parents = int(rng.integers(1, N + 1))
        replace = int(rng.integers(0, N - parents + 1))
        src, rank = both(scores, parents, replace, None if eligible is None else eligible.tolist())
        replaced = [e for e in range(E) if src[e] != e]
        assert len(replaced) == replace
        assert all(src[src[e]] == src[e] for e in range(E)), "a source is replaced"
        assert set(src[e] for e in replaced) <= set(rank[:parents]) and not set(replaced) & set(rank[:parents])
        assert all(eligible is None or eligible[e] for e in replaced)


def refused(lib, *args):
    assert lib.frirl_hip_select_plan(*args) == EINVAL
    return lib.frirl_hip_last_error().decode()


def test_every_refusal_names_its_cause(lib):
    E = 4
    sc = (frirl_amd.RolloutScore * E)()
    src = (C.c_int32 * E)(*([77] * E))
    assert "NULL" in refused(lib, None, E, None, 1, 1, src, None)
    assert "NULL" in refused(lib, sc, E, None, 1, 1, None, None)
    assert "E=0" in refused(lib, sc, 0, None, 1, 1, src, None)
    assert "parents=0" in refused(lib, sc, E, None, 0, 1, src, None)
    assert "replace=-1" in refused(lib, sc, E, None, 1, -1, src, None)
    msg = refused(lib, sc, E, None, 2, 3, src, None)
    assert "parents=2" in msg and "replace=3" in msg and "4 eligible" in msg
    mask = (C.c_uint8 * E)(1, 0, 1, 1)
    assert "3 eligible" in refused(lib, sc, E, mask, 2, 2, src, None)
    sc[2].reward_sum = float("nan")
    assert "agent 2" in refused(lib, sc, E, None, 1, 1, src, None) and "NaN" in lib.frirl_hip_last_error().decode()
    assert list(src) == [77] * E, "a refused plan writes nothing"
    mask = (C.c_uint8 * E)(1, 1, 0, 1)                      # a NaN of an agent that takes no part is nobody's business
    assert lib.frirl_hip_select_plan(sc, E, mask, 1, 1, src, None) == 0
    with pytest.raises(frirl_amd.FrirlHipError, match="parents=3"):
        frirl_amd.select_plan([(0, 0.0)] * 3, 3, 1)


def test_clone_agents_checks_its_arguments_before_the_device(lib):
    """NULL b / rb / nrules / src, nant outside 2..9, E < 1, odd maxR, misaligned rows: FRIRL_HIP_EINVAL (-2) where a machine without
    a GPU would otherwise answer FRIRL_HIP_ENODEV (-1)."""
    buf = (C.c_double * 64)()
    base = C.addressof(buf)
    base += (-base) % 16

    def call(E=3, maxR=4, nant=3, rb=base, nrules=base, uidx=None, src=base, b=True, envs=None, conv=None, weights=None):
        rbs = frirl_amd.RuleBases(E, maxR, rb, nrules, uidx)
        return lib.frirl_hip_clone_agents(C.byref(rbs) if b else None, nant, envs, conv, weights, src, None, None)

    for kw, word in ((dict(b=False), "NULL"), (dict(rb=None), "NULL"), (dict(nrules=None), "NULL"), (dict(src=None), "NULL"), (dict(nant=1), "nant=1"),
                     (dict(nant=10), "nant=10"), (dict(E=0), "E=0"), (dict(maxR=5), "maxR=5"), (dict(rb=base + 8), "16-byte"), (dict(weights=base + 8), "16-byte"),
                     (dict(uidx=base + 2), "4-byte")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.frirl_hip_last_error().decode(), (kw, lib.frirl_hip_last_error())
    conv = frirl_amd.ConvergenceDesc(base, base, base, None, base, base, None)
    assert call(conv=C.byref(conv)) == EINVAL and "conv" in lib.frirl_hip_last_error().decode()
    envs = frirl_amd.EnvsDesc()
    envs.rant = base + 8
    assert call(envs=C.byref(envs)) == EINVAL and "envs->rant" in lib.frirl_hip_last_error().decode()
