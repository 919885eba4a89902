"""Every rung of the persistent learner's launch table (csrc/learn_kernel.h: FRIRL_LEARN_SHAPES x the levels plain / ROWS / EXPLORE /
TARGET) at every lane-group size: the three demos at 1, 2, 4, 8, 16, 32 and 64 lanes per agent, and at each size the four levels on the
same work -- level 0 with no struct, levels 1 .. 3 each selected by its own struct alone, filled so that it asks for nothing.  A non-NULL
struct pointer is what picks a level, so each run reaches its own kernels, and all four must leave the same bytes.

The tests of the levels (test_hip_learn.py, test_hip_hparam_rows.py, test_hip_explore_rows.py, test_hip_target.py) hold the kernels to
the oracle's chains at 1 and 64 lanes and assert these equivalences at the default size; this one walks the table.

Bar: every state array byte for byte (tests/test_hip_external.py: assert_same)."""
import numpy as np
import pytest

import frirl_amd
from tests import explore_rows_cases as xc
from tests import hparams_cases as hc

gpu = pytest.mark.gpu
E = 5                   # 16 lanes per agent: 4 agents in a wave, the fifth opens a second tile; 64 lanes: an agent is a wave
SLICES = (1, 2, 4, 8, 16, 32, 64)
DEMOS = ("mountaincar", "acrobot", "cartpole")


def neutral_structs(dev0):
    """what selects level 0 .. 3 and changes nothing: no struct; hyper-parameter rows with every column NULL; exploration rows with no
    column and horizon 0; a target struct that gives every agent SARSA"""
    return (dict(), dict(rows=frirl_amd.HparamRows(E, dev0)), dict(explore=frirl_amd.ExploreRows(E, dev0)),
            dict(target=frirl_amd.TargetRows(E, dev0, target_all=frirl_amd.TARGET_SARSA)))


@gpu
@pytest.mark.parametrize("env,slices", [(env, s) for env in DEMOS for s in SLICES if (env, s) != ("cartpole", 1)])      # cartpole at 1 runs at 2
def test_every_level_of_every_rung_leaves_the_plain_learners_bytes(env, slices, hip_option):
    """5 greedy agents from start states spread over the state grids, at most 3 episodes, frirl_hip_learn_train against _train_rows,
    _train_explore and _train_target with neutral structs at `slices` lanes per agent: every state array byte for byte the same, at
    least one launch, and every agent ran an episode (a rung that resolves to no launch cannot pass by being empty four times)."""
    import torch
    from tests.test_hip_external import assert_same
    from tests.test_hip_hparam_rows import learner_state
    dev0 = torch.device("cuda", 0)
    hip_option("learn_slices", slices)
    d = hc.demo_desc(env, "default")
    rng = np.random.default_rng(17)
    start = torch.from_numpy(np.ascontiguousarray(np.stack([rng.choice(d["grids"][k], E) for k in range(d["nstates"])], 1))).to(dev0)
    outs = []
    for level, kw in enumerate(neutral_structs(dev0)):
        prob, agent, envs = frirl_amd.fresh_batch(d, E, xc.MAXR, dev0, start_states=start, no_random=1)
        run = frirl_amd.train_persistent(prob, agent, envs, max_episodes=3, budget=700, **kw)
        torch.cuda.synchronize()
        assert run.launches >= 1 and bool((run.conv.episodes > 0).all()), (level, run.launches, run.conv.episodes.tolist())
        outs.append(learner_state(prob, envs, run))
    for level in (1, 2, 3):
        assert_same(outs[0], outs[level], ("level", level))
