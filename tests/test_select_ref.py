"""The selection cases of tests/select_cases.py on the oracle alone (no GPU): every chain keeps the greedy picks apart, none converges,
and each ends somewhere else than the plain runs of either set -- without which the device test could not tell a missing clone or a
wrongly inherited row from the right result."""
import pytest

from tests import hparams_cases as hc
from tests import select_cases as sc


@pytest.mark.parametrize("env,a,b,k,m", sc.CASES)
def test_chain_cases_are_admitted(env, a, b, k, m):
    """min_gap measured (portable trig, maxR = 512): mountaincar thr_small -> noskip_thr_small_tight 4.8e-6, the reverse 3.2e-6, default
    -> thr_small 7.1e-6, thr_small -> default 5.0e-6; acrobot noskip -> thr_big 5.4e-5, alpha_gamma -> thr0 7.0e-6, thr_big -> noskip
    3.0e-4, default -> alpha_gamma 1.0e-4; cartpole noskip -> thr_small 3.3e-6."""
    assert (k, m) == sc.EPISODES[env]
    run = sc.chain(env, a, b, k, m)
    print(env, a, b, "min_gap", run["stats"]["min_gap"], "records", run["records"])
    assert run["stats"]["min_gap"] >= hc.MIN_GAP
    assert run["converged"] == 0 and len(run["records"]) == k + m
    assert run["fr"].five.R < sc.MAXR
    # the source of the clone (a all the way) and the agent the clone would be without the clone (b all the way) qualify too
    for plain in (sc.chain(env, a, a, k, m), sc.chain(env, b, b, k, m)):
        assert plain["stats"]["min_gap"] >= hc.MIN_GAP and plain["converged"] == 0
        assert sc.final(plain) != sc.final(run), "the chain cannot be told from a plain run"
    # and the k episodes under b that the clone loses differ from the k under a it takes over
    assert sc.chain(env, a, a, k, m)["records"][:k] != sc.chain(env, b, b, k, m)["records"][:k]


@pytest.mark.parametrize("env", sc.ENVS)
def test_the_untouched_agent_is_an_admitted_plain_case(env):
    name, (k, m) = sc.UNTOUCHED[env], sc.EPISODES[env]
    assert (env, name) in hc.TRAJ_CASES and k + m + 1 <= hc.TRAJ_EPISODES[env]
    run = sc.chain(env, name, name, k, m)
    assert run["stats"]["min_gap"] >= hc.MIN_GAP and run["converged"] == 0


@pytest.mark.parametrize("env", sc.ENVS)
def test_a_chain_of_single_episodes_under_one_set_is_the_plain_run(env):
    """chain(a, a) against one run(max_episodes = k + m + 1): the same final state, so the chains measure the switch and nothing else."""
    name, (k, m) = sc.UNTOUCHED[env], sc.EPISODES[env]
    whole = hc.demo_frirl(env, name, trig_mode=1, maxR=sc.MAXR)
    assert whole.run(max_episodes=k + m + 1) == 0
    assert sc.final(dict(fr=whole)) == sc.final(sc.chain(env, name, name, k, m))
