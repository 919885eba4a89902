"""Reference and fixtures of the imitation tests: a per-agent mirror that takes a teacher's actions (reference frirl_episode.c:58-79,
127-151: keyaction replaces the epsilon-greedy action) and replays recorded logs record by record, and seeded generators of such logs.
No GPU needed.

A log is what frirl_hip_learn_demonstration reads (include/frirl_hip.h: struct frirl_hip_demonstration), as numpy arrays for E agents:
obs [E, T, ns], q_obs [E, T, ns] or None, action [E, T] int32, reward [E, T], success [E, T] int32, start [E, T] uint8, length [E]
int32; records past length[e] are padding.  Every generated log is a sequence of episodes of a scripted teacher, built so that it holds
an episode ended by success (with records after its end: they must be skipped), one cut short by the next start and one run to
max_steps.
"""
import functools

import numpy as np

import frirl_amd
from oracle import binding as ob
from tests import hparams_cases
from tests.test_hip_external import Mirror, PointEnv, generic_quantize, point_desc

INACTIVE, EXACT, SPREAD, INSERTED, SKIPPED, FULL = (frirl_amd.UPD_INACTIVE, frirl_amd.UPD_EXACT, frirl_amd.UPD_SPREAD, frirl_amd.UPD_INSERTED,
                                                    frirl_amd.UPD_SKIPPED, frirl_amd.UPD_FULL)


class TaughtMirror(Mirror):
    """Mirror whose pick is the teacher's where the teacher names an action (teacher: callable(step) -> index; anything outside
    0..A-1 = "choose yourself"), plus the per-record replay of a log as include/frirl_hip.h specifies it."""

    def __init__(self, d, start, maxR, p=0, explore=None, gid=0, teacher=None):
        super().__init__(d, start, maxR, p=p, explore=explore, gid=gid)
        self.teacher, self.A = teacher, len(d["grids"][-1])
        self.taught = 0
        # state of the replay: what frirl_hip_envs row e holds
        self.done, self.steps, self.total, self.status, self.refused = 0, 0, 0.0, INACTIVE, 0
        self.states = self.q_ant = None
        self.branches = {s: 0 for s in (EXACT, SPREAD, INSERTED, SKIPPED, FULL)}
        self.same_point = 0        # steps whose (s', a') equals (s, a): the replay kernel's one-conclusion form
        self.skipped = 0           # records skipped because the episode had ended
        self.trace = []            # status after every consumed record

    def pick(self, states, device_pick, step=0):
        k = self.teacher(step) if self.teacher is not None else -1
        if 0 <= k < self.A:
            self.taught += 1
            return int(k)
        return super().pick(states, device_pick, step)

    def learn(self, q_ant, reward, cur_q_ant):
        """One frirl_update_sarsa with the capacity rule of the device: an append at a full rule base is refused and changes nothing
        (FRIRL_HIP_UPD_FULL).  Returns the status the device reports; the update itself is the oracle's."""
        f, oa = self.five, self.oa
        status = hparams_cases.classify(f, oa, self.fus, q_ant, reward, cur_q_ant)
        if status == INSERTED and f.R >= f.maxR:
            return FULL
        self.fus = f.update_sarsa(oa, self.fus, q_ant, reward, cur_q_ant)
        return status

    def replay(self, log, e, passes=1):
        """Agent e's log, record by record.  Returns the number of records consumed."""
        d, av = self.d, self.d["grids"][-1]
        src = e if log["obs"].shape[0] > 1 else 0
        consumed = 0
        for _ in range(passes):
            for r in range(int(log["length"][e])):
                a = int(log["action"][src, r])
                if not 0 <= a < self.A:
                    return consumed
                obs = log["obs"][src, r]
                if r == 0 or log["start"][src, r]:
                    self.episode_no += 1
                    self.states, self.q_ant = obs.copy(), np.concatenate([obs, [av[a]]])
                    self.done, self.steps, self.total, self.status = 0, 0, 0.0, INACTIVE
                elif self.done:
                    self.status = INACTIVE
                    self.skipped += 1
                else:
                    q = log["q_obs"][src, r] if log["q_obs"] is not None else generic_quantize(d, obs)
                    cur_q_ant = np.concatenate([q, [av[a]]])
                    reward = float(log["reward"][src, r])
                    self.same_point += int((cur_q_ant == self.q_ant).all())
                    self.status = self.learn(self.q_ant, reward, cur_q_ant)
                    self.branches[self.status] += 1
                    self.refused |= int(self.status == FULL)
                    self.states, self.q_ant = obs.copy(), cur_q_ant
                    self.steps += 1
                    self.total += reward
                    if int(log["success"][src, r]) == 1 or self.steps >= d["max_steps"]:
                        self.done = 1
                consumed += 1
                self.trace.append(self.status)
        return consumed


# ---- logs -------------------------------------------------------------------------------------------------------------------
class LogWriter:
    """Episodes of one agent, appended record by record."""

    def __init__(self, ns, with_q):
        self.obs, self.q, self.action, self.reward, self.success, self.start = [], [], [], [], [], []
        self.ns, self.with_q = ns, with_q
        self.ends = []          # per episode: "success", "max_steps" or "cut", and its number of steps

    def episode(self, step_fn, start, teacher, max_steps, cut=None, tail=0):
        """step_fn(x, action index) -> (x', reward, success, q' or None); teacher(x, t) -> action index.  Runs until success or
        max_steps (or `cut` steps), then `tail` more records the replay must skip."""
        x = np.array(start, dtype=np.float64)
        self._put(x, np.zeros(self.ns), teacher(x, 0), 0.0, 0, 1)
        t, end = 0, "cut"
        while cut is None or t < cut:
            x, r, ok, q = step_fn(x, self.action[-1])
            t += 1
            self._put(x, q, teacher(x, t), r, ok, 0)
            if ok == 1 or t >= max_steps:
                end = "success" if ok == 1 else "max_steps"
                break
        self.ends.append((end, t))
        for j in range(tail):
            x, r, ok, q = step_fn(x, self.action[-1])
            self._put(x, q, teacher(x, t + 1 + j), r, 0, 0)

    def _put(self, x, q, a, r, ok, start):
        self.obs.append(np.array(x))
        self.q.append(np.zeros(self.ns) if q is None else np.array(q))
        self.action.append(int(a))
        self.reward.append(float(r))
        self.success.append(int(ok))
        self.start.append(int(start))


def pack_logs(writers, with_q):
    E, T, ns = len(writers), max(len(w.action) for w in writers), writers[0].ns
    log = dict(obs=np.zeros((E, T, ns)), q_obs=np.zeros((E, T, ns)) if with_q else None, action=np.zeros((E, T), dtype=np.int32),
               reward=np.zeros((E, T)), success=np.zeros((E, T), dtype=np.int32), start=np.zeros((E, T), dtype=np.uint8),
               length=np.array([len(w.action) for w in writers], dtype=np.int32), ends=[w.ends for w in writers])
    for e, w in enumerate(writers):
        n = len(w.action)
        log["obs"][e, :n], log["action"][e, :n], log["reward"][e, :n] = np.array(w.obs), w.action, w.reward
        log["success"][e, :n], log["start"][e, :n] = w.success, w.start
        if with_q:
            log["q_obs"][e, :n] = np.array(w.q)
    return log


POINT_MAX_STEPS = 60


@functools.lru_cache(maxsize=None)
def point_case(nant, A, E=8, maxR=512, seed=0, hparams="default"):
    """PointEnv logs of a proportional controller with seeded deviations: (description, logs).  The controller takes the action that
    brings the next state closest to the origin; one pick in seven is a seeded random action instead.  hparams: a set of
    tests/hparams_cases.py applied to the description (the logs are the scripted teacher's and do not depend on it)."""
    base = point_desc(nant, A)
    d = dict(base, max_steps=POINT_MAX_STEPS, **hparams_cases.overrides(hparams, base, point=True))
    env, av, ns = PointEnv(nant - 1), point_desc(nant, A)["grids"][-1], nant - 1
    gain = np.array(env.gain)
    writers = []
    for e in range(E):
        rng = np.random.default_rng(1000 * nant + 10 * A + 7919 * seed + e)

        def step_fn(x, a):
            x2, r, ok = env.step(np, x[None], np.array([av[a]]))
            return x2[0], float(r[0]), int(ok[0]), None

        def controller(x, t):
            if rng.uniform() < 1.0 / 7.0:
                return int(rng.integers(A))
            want = -(0.95 * x * gain).sum() / (gain * gain).sum()
            return int(np.argmin(np.abs(av - want)))

        def away(x, t):
            return A - 1 if (x * gain).sum() >= 0 else 0

        def start():            # outside the goal region in every coordinate
            return rng.uniform(0.3, 0.6, ns) * rng.choice([-1.0, 1.0], ns)

        w = LogWriter(ns, False)
        w.episode(step_fn, start(), controller, POINT_MAX_STEPS, tail=3)          # to its end, then records to skip
        w.episode(step_fn, rng.uniform(0.75, 0.9, ns) * rng.choice([-1.0, 1.0], ns), controller, POINT_MAX_STEPS, cut=4)     # cut short by the next start
        w.episode(step_fn, start(), away, POINT_MAX_STEPS)                        # pushed away from the goal: runs to max_steps
        w.episode(step_fn, start(), controller, POINT_MAX_STEPS)
        writers.append(w)
    return d, pack_logs(writers, False)


DEMO_MAX_STEPS = 80


def demo_teacher(env, A):
    if env == "mountaincar":
        return lambda x, t: 2 if x[1] >= 0 else 0
    if env == "acrobot":
        return lambda x, t: 2 if x[2] + x[3] >= 0 else 0
    # cartpole: a clipped linear law on (x, x', theta, theta'), in units of a tenth of the full force
    return lambda x, t: int(min(max(round(A // 2 + 10.0 * (0.1 * x[0] + 0.3 * x[1] + 6.0 * x[2] + 0.9 * x[3])), 0), A - 1))


# start states from which the scripted teacher ends the episode well inside DEMO_MAX_STEPS, and its idle counterpart
DEMO_SHORT_START = {"mountaincar": [-1.1, 0.0], "acrobot": [1.2, 0.0, 2.5, 0.0], "cartpole": [0.0, 0.0, 0.15, 0.0]}


@functools.lru_cache(maxsize=None)
def demo_case(env, E=8):
    """Logs of the three demos' scripted teachers through the oracle's environment and quantiser: (description, logs)."""
    d = dict(frirl_amd.demo_describe(env), max_steps=DEMO_MAX_STEPS)
    fr = ob.Frirl(env)
    av, A, ns = d["grids"][-1], d["A"], d["nstates"]
    good = demo_teacher(env, A)
    writers = []
    for e in range(E):
        rng = np.random.default_rng(4000 + e)

        def step_fn(x, a):
            x2, r, ok, q = fr.env_step(av[a], x)
            return x2, r, ok, q

        def noisy(x, t):
            return int(rng.integers(A)) if rng.uniform() < 0.1 else good(x, t)

        jitter = lambda s: np.array(s) * (1.0 + 0.02 * rng.uniform(-1, 1, ns))      # noqa: E731
        w = LogWriter(ns, True)
        first = jitter(DEMO_SHORT_START[env])
        if env == "cartpole":       # "success" is the pole falling: a full push ends the episode, the linear law runs to max_steps
            w.episode(step_fn, first, lambda x, t: A - 1, DEMO_MAX_STEPS, tail=3)
            w.episode(step_fn, jitter(DEMO_SHORT_START[env]), noisy, DEMO_MAX_STEPS, cut=7)
            w.episode(step_fn, d["values_def"][:ns] + 0.01 * rng.uniform(-1, 1, ns), good, DEMO_MAX_STEPS)
        else:
            w.episode(step_fn, first, noisy, DEMO_MAX_STEPS, tail=3)
            w.episode(step_fn, d["values_def"][:ns] + 0.01 * rng.uniform(-1, 1, ns), noisy, DEMO_MAX_STEPS, cut=7)
            w.episode(step_fn, d["values_def"][:ns] + 0.01 * rng.uniform(-1, 1, ns), lambda x, t: 1, DEMO_MAX_STEPS)     # idle: runs to max_steps
        # the first start state again: its rule place exists by now, so the un-quantised start point is updated by a weighted spread
        w.episode(step_fn, first, noisy, DEMO_MAX_STEPS, cut=5)
        writers.append(w)
    return d, pack_logs(writers, True)


def mirrors_for(d, log, maxR, p=0):
    return [TaughtMirror(d, log["obs"][e if log["obs"].shape[0] > 1 else 0, 0], maxR, p=p, gid=e) for e in range(len(log["length"]))]
