"""Hyper-parameter sets off the demos' values (alpha, gamma, the qdiff insertion bounds, the spread threshold weight_significant,
skip_rules) and the CPU side of the tests that use them: the cases, the oracle's own runs of them and the conditions under which a
case is worth running on the device.  No GPU needed; tests/test_hparams_ref.py asserts every condition on the oracle alone.

A set is a function of the description's own values, so that "tight bounds" or "half the learning rate" mean the same on every
demo.  Keys are those of oracle.binding.Frirl.hparams and of the description dicts of frirl_amd.describe / demo_describe.
"""
import functools

import numpy as np

from oracle import binding as ob

ENVS = ["mountaincar", "cartpole", "acrobot"]


def _combined(h, point):
    return dict(skip_rules=0, weight_thr=0.002, qdiff_pos=h["qdiff_pos"] * 0.25, qdiff_neg=h["qdiff_neg"] * (0.5 if point else 0.25))


SETS = {
    "default": lambda h, point: {},
    "noskip": lambda h, point: dict(skip_rules=0),
    "thr0": lambda h, point: dict(weight_thr=0.0),
    "thr_small": lambda h, point: dict(weight_thr=0.002),
    "thr_big": lambda h, point: dict(weight_thr=0.3),
    "noskip_thr_small_tight": _combined,
    "alpha_gamma": lambda h, point: dict(alpha=1.0, gamma=0.9) if point else dict(alpha=h["alpha"] * 0.5, gamma=0.9),
    "never_insert": lambda h, point: dict(qdiff_pos=1e30, qdiff_neg=-1e30),
}
NON_DEFAULT = [s for s in SETS if s != "default"]
HP_KEYS = ("alpha", "gamma", "qdiff_pos", "qdiff_neg", "weight_thr", "skip_rules")


def overrides(name, h, point=False):
    """The fields the set `name` changes, given the description's own values h (any mapping with HP_KEYS)."""
    return SETS[name](h, point)


def demo_frirl(env, name, trig_mode=1, maxR=0):
    """The oracle's demo agent with the set applied."""
    fr = ob.Frirl(env, trig_mode=trig_mode, maxR=maxR)
    fr.set_hparams(**overrides(name, fr.hparams))
    return fr


def demo_desc(env, name):
    """frirl_amd.demo_describe(env) with the set applied."""
    import frirl_amd
    d = frirl_amd.demo_describe(env)
    return dict(d, **overrides(name, d))


def point_desc(nant, A, name):
    """tests/test_hip_external.py::point_desc with the set applied (the point shapes' values: 0.5 / 1.0 / +-1.0 / 0.05 / 1)."""
    from tests.test_hip_external import point_desc as base
    d = base(nant, A)
    return dict(d, **overrides(name, d, point=True))


# ---- 1. the genuine reference's runs (fixtures under tests/golden/hparams/, written by oracle/make_golden.py) ----------------------
# (env, set, episodes): skip_rules = 0 on every demo, the small and the large threshold on one demo each, the combined set on one
REF_CASES = [("mountaincar", "noskip", 12), ("cartpole", "noskip", 8), ("acrobot", "noskip", 8), ("cartpole", "thr_small", 8),
             ("acrobot", "thr_big", 8), ("mountaincar", "noskip_thr_small_tight", 12)]


def ref_case_values(env, name):
    """The six values the reference harness takes for a case, in its argument order."""
    h = demo_frirl(env, name, trig_mode=0).hparams
    return [h[k] for k in HP_KEYS]


# ---- 2. whole trajectories with greedy picks inside the kernel --------------------------------------------------------------------
# (env, set, max_episodes) admitted for the kernels that pick the greedy action themselves: the oracle's own run keeps a relative gap
# of at least MIN_GAP between its two best conclusions at every pick (explore_stats["min_gap"]), so that a device sum that differs
# in the last bits takes the same action.  Measured by tests/test_hparams_ref.py::test_trajectory_cases_are_admitted (portable trig,
# maxR = 512): see its docstring for min_gap, rules and steps per case.
MIN_GAP = 1e-6
TRAJ_EPISODES = {"mountaincar": 14, "acrobot": 8, "cartpole": 6}
TRAJ_CASES = [
    ("mountaincar", "thr_small"), ("mountaincar", "noskip_thr_small_tight"),
    ("acrobot", "noskip"), ("acrobot", "thr0"), ("acrobot", "thr_big"), ("acrobot", "alpha_gamma"), ("acrobot", "never_insert"),
    ("cartpole", "noskip"), ("cartpole", "thr_small"), ("cartpole", "thr_big"), ("cartpole", "noskip_thr_small_tight"), ("cartpole", "alpha_gamma"),
]
TRAJ_MAXR = 512


@functools.lru_cache(maxsize=None)
def traj_run(env, name, max_episodes=None):
    """The oracle's construct run of a trajectory case (at most max_episodes - 1 episodes): dict(fr, converged, episodes, total_steps,
    stats = explore_stats, spread = the rule base's spread_stats).  Cached: the Frirl object is shared, read it only."""
    fr = demo_frirl(env, name, trig_mode=1, maxR=TRAJ_MAXR)
    converged = fr.run(max_episodes=max_episodes or TRAJ_EPISODES[env])
    episodes = int(ob.lib().orc_frirl_episode_num(fr.h)) - (0 if converged else 1)          # the counter stops on the episode that converged
    return dict(fr=fr, converged=converged, episodes=episodes, total_steps=fr.total_steps,
                stats=fr.explore_stats, spread=fr.five.spread_stats)


# ---- 3. update level ----------------------------------------------------------------------------------------------------------------
EXACT, SPREAD, INSERTED, SKIPPED = 1, 2, 3, 4          # the values of FRIRL_HIP_UPD_EXACT ... _SKIPPED (include/frirl_hip.h)
UPDATE_TABLES = [("mountaincar", 6), ("cartpole", 9), ("acrobot", 5), ("point", (2, 3)), ("point", (8, 3))]
UPDATE_TABLE_IDS = ["mountaincar", "cartpole", "acrobot", "point2x3", "point8x3"]
ROUNDS = 6          # random rounds; then crafted rounds A and B


class Table:
    """A grown rule base with its tables, grids and an oracle agent description: what an update-level case starts from."""

    def __init__(self, five, grids, h, A, env_kind_source, action_ve, grid_div):
        f = five
        self.action_ve, self.grid_div = np.array(action_ve), np.array(grid_div)
        self.nant, self.U, self.A, self.R = f.nant, f.U, A, f.R
        self.u, self.ve = np.array(f.u), np.array(f.ve)
        self.rant = np.array(f.rant[: f.R])
        self.veval = np.array(f.veval[:, : f.R])
        self.uidx = np.array(f.uidx[:, : f.R])
        self.rconc = np.array(f.rconc[: f.R])
        self.grids, self.h, self.source = [np.array(g) for g in grids], dict(h), env_kind_source
        # points of the state universes (also outside the rule grid) at which many rules carry a Shepard weight above 0.002: the 8 best
        # of 400 seeded candidates, counted by the oracle
        rng = np.random.default_rng(77)
        cand = np.array([[rng.uniform(self.u[k, 0], self.u[k, -2]) for k in range(self.nant - 1)] + [self.grids[-1][rng.integers(A)]] for _ in range(400)])
        count = []
        for x in cand:
            hit = f.vag_concl_weight(x)
            count.append(int((np.array(f.weights[: f.R]) > 0.002).sum()) if hit < 0 else 0)
        self.wide_points = cand[np.argsort(count, kind="stable")[-8:]]


@functools.lru_cache(maxsize=None)
def update_table(kind, arg):
    if kind == "point":
        from tests.test_hip_external import Mirror, PointEnv, point_desc as base
        nant, A = arg
        d = base(nant, A)
        m = Mirror(d, np.full(nant - 1, 0.55), 1024)
        for _ in range(3):                      # the oracle alone grows the corner rule base
            m.episode(PointEnv(nant - 1), None)
        return Table(m.five, d["grids"], {k: d[k] for k in HP_KEYS}, A, d, d["action_ve"], d["grid_div"])
    fr = ob.Frirl(kind)
    fr.run(max_episodes=arg + 1)
    return Table(fr.five, [fr.dim(k)["values"] for k in range(fr.nant)], fr.hparams, fr.nactions, fr, fr.action_vevalues,
                 [fr.dim(k)["values_div"] for k in range(fr.nant)])


def classify(f, oa, fus, q_ant, reward, cur):
    """Branch of frirl_update_sarsa (reference frirl_update_sarsa.c:348-385, update_rules :22-63) the oracle takes for this update,
    before it is applied: f an ob.Five, oa an ob.Agent, fus the sticky flag.  The one restatement the tests share
    (tests/teach_ref.py::TaughtMirror.learn adds the device's capacity rule to it)."""
    _, qp = f.vag_concl(cur)
    hit, qnow = f.vag_concl(q_ant)
    qdiff = oa.alpha * (reward + oa.gamma * qp - qnow)
    if qdiff > oa.qdiff_pos or qdiff < oa.qdiff_neg:
        snapped = [ob.lib().orc_check_possible_states(float(q_ant[i]), ob.dp(oa.grids[i]), len(oa.grids[i])) for i in range(len(q_ant))]
        if f.vag_concl(snapped)[0] < 0:
            return INSERTED
        fus = 0
    rules = f.R - (1 if fus else 0)
    if hit >= 0 and (oa.skip_rules == 0 or hit < rules):
        return EXACT
    if oa.skip_rules == 1 and hit >= 0 and hit == rules:
        return SKIPPED
    return SPREAD


class UpdateCase:
    """Eight rounds of E independent updates on copies of a table, run on the oracle: per round the inputs and what every
    environment must hold afterwards.  Rounds 0..5 draw as tests/test_hip_sarsa.py does; rounds A and B query the rule an environment
    has just inserted (sticky flag set) with a qdiff inside, then outside the insertion bounds."""

    def __init__(self, table, name, E, seed=11):
        t = table
        point = not isinstance(t.source, ob.Frirl)
        h = dict(t.h, **overrides(name, t.h, point=point))
        self.h, self.E, self.table, self.name = h, E, t, name
        self.maxR = t.R + 64 + ((t.R + 64) & 1)
        oa = ob.Agent(h["alpha"], h["gamma"], h["qdiff_pos"], h["qdiff_neg"], h["weight_thr"], h["skip_rules"], t.grids)
        self.fives = [ob.Five(t.u.ravel(), t.ve.ravel(), t.nant, t.U, self.maxR, t.rant, t.rconc.copy()) for _ in range(E)]
        # every third environment starts as if its last rule had just been inserted
        self.fus0 = np.array([1 if e % 3 == 0 else 0 for e in range(E)], dtype=np.int32)
        fus = self.fus0.astype(np.float64)
        rng = np.random.default_rng(seed)
        nant = t.nant
        self.rounds = []
        self.seen = set()
        for rnd in range(ROUNDS + 2):
            q_ant, cur, reward = np.zeros((E, nant)), np.zeros((E, nant)), np.zeros(E)
            crafted = np.zeros(E, dtype=bool)
            for e in range(E):
                for k in range(nant):
                    v = t.grids[k]
                    q_ant[e, k] = v[rng.integers(len(v))]
                    cur[e, k] = v[rng.integers(len(v))]
                if e % 7 == 5:      # a rule of the table: an exact hit whatever was inserted since
                    q_ant[e] = t.rant[rng.integers(t.R)]
                if e % 5 == 3:      # off-grid state: Shepard spread / snapped insert
                    for k in range(nant - 1):
                        v = t.grids[k]
                        q_ant[e, k] = rng.uniform(v[0], v[-1]) * 0.9
                if e % 10 == 8:     # a point whose spread reaches many rules at a small threshold
                    q_ant[e] = t.wide_points[rng.integers(len(t.wide_points))]
                reward[e] = [-10.0, 1000.0, -3000.0 * rng.random(), 20 * rng.random() - 10][e % 4]
                if rnd >= ROUNDS and fus[e] and e != E - 1:
                    f = self.fives[e]
                    crafted[e] = True
                    q_ant[e] = f.rant[f.R - 1]
                    qnow, qp = f.vag_concl(q_ant[e])[1], f.vag_concl(cur[e])[1]
                    if rnd == ROUNDS:            # A: qdiff strictly inside the bounds
                        reward[e] = qnow - h["gamma"] * qp + 0.1 * min(h["qdiff_pos"], -h["qdiff_neg"]) / h["alpha"]
                    elif h["qdiff_pos"] < 1e29:  # B: outside, above or below (never_insert has no outside: the drawn reward stays)
                        reward[e] = qnow - h["gamma"] * qp + 3.0 * (h["qdiff_pos"] if e % 2 else h["qdiff_neg"]) / h["alpha"]
            active = np.ones(E, dtype=np.uint8)
            active[E - 1] = 0
            status, R, rconc, new_rule = [], np.zeros(E, dtype=np.int32), [], {}
            for e in range(E):
                f = self.fives[e]
                if not active[e]:
                    status.append(None)
                    R[e] = f.R
                    rconc.append(np.array(f.rconc[: f.R]))
                    continue
                Rb, before = f.R, np.array(f.rconc[: f.R])
                st = classify(f, oa, fus[e], q_ant[e], reward[e], cur[e])
                fus[e] = f.update_sarsa(oa, fus[e], q_ant[e], reward[e], cur[e])
                assert (f.R > Rb) == (st == INSERTED)
                if st == INSERTED:
                    new_rule[e] = (np.array(f.rant[Rb]), np.array(f.veval[:, Rb]), np.array(f.uidx[:, Rb]))
                if st == SKIPPED:
                    assert (np.array(f.rconc[: f.R]) == before).all()
                status.append(st)
                self.seen.add(st)
                R[e] = f.R
                rconc.append(np.array(f.rconc[: f.R]))
            self.rounds.append(dict(q_ant=q_ant, cur=cur, reward=reward, active=active, crafted=crafted, status=status, R=R, rconc=rconc,
                                    fus=fus.astype(np.int32).copy(), new_rule=new_rule))
        st = [f.spread_stats for f in self.fives]
        self.moved_max = max(x["moved_max"] for x in st)                       # most rules one spread wrote
        self.moved_min = min(x["moved_min"] for x in st if x["spreads"])       # fewest


@functools.lru_cache(maxsize=None)
def update_case(table_index, name, E):
    kind, arg = UPDATE_TABLES[table_index]
    return UpdateCase(update_table(kind, arg), name, E)


# ---- 4c. caller-stepped agents on the point shapes ----------------------------------------------------------------------------------
EXTERNAL_SHAPES = [(4, 5), (5, 11), (8, 3)]


# ---- 4d. demonstration replay -------------------------------------------------------------------------------------------------------
TEACH_SHAPES = [(4, 3), (6, 11)]
TEACH_SETS = ["noskip", "thr_small", "thr_big", "noskip_thr_small_tight"]
