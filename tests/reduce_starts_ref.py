"""CPU model of the reduction against a set of start states (frirl_hip_reduce_batch_starts, DESIGN "Reduction against a set of start
states") over the oracle: the reference's try-remove loop (frirl_sequential_run.c:170-350) with every trial replayed from K start
states and a removal accepted iff the acceptance test (:212) holds for ALL of them, prev_reward carried per start (:222).

Two forms that must agree: `sequential` (one candidate per trial, as the reference) and `tree_walk` (the accept/reject tree of the next
`depth` candidates, every node replayed from every used start, walked along the outcomes that happened -- what the device runs).
The replays go through tests/test_hip_reduce_batch.py's Trained (restore / set_start_state / episode_eval).  With K = 1 and
drop_bad_starts = False `sequential` is the oracle's own fr.reduce (tests/test_reduce_starts_ref.py)."""
import numpy as np


class Replayer:
    """Greedy replays of subsets of ONE trained rule base (a Trained of tests/test_hip_reduce_batch.py) from any start state.  The
    rule base inside the oracle is rebuilt only when the requested subset is not the current one minus a single rule.  The oracle is
    shared with other tests, and fr.dim(k)["values_def"] reads its CURRENT start state: every replay puts the agent's own start state
    back, and done() the whole rule base."""

    def __init__(self, trained):
        self.t = trained
        self.good_above = trained.fr.hparams["reward_good_above"]
        self.current = None

    def set_rules(self, idx):
        idx = list(idx)
        f = self.t.fr.five
        cur = self.current
        if cur is not None and len(cur) == len(idx) + 1:
            i = 0
            while i < len(idx) and cur[i] == idx[i]:
                i += 1
            if cur[:i] + cur[i + 1:] == idx:
                f.remove_rule(i)                                     # keeps the order of the others (five_remove_rule)
                self.current = idx
                return
        if cur != idx:
            self.t.restore(self.t.rant[idx], self.t.rconc[idx])
            self.current = idx

    def replay(self, idx, start):
        """(steps, reward) of the greedy episode on the rules `idx` (original indices, ascending) from `start`"""
        self.set_rules(idx)
        self.t.fr.set_start_state(start)
        self.t.fr.episode_eval()
        self.t.fr.set_start_state(self.t.start)
        return self.t.fr.ep_steps, self.t.fr.ep_reward

    def done(self):
        self.set_rules(range(self.t.R0))


def accept(steps, reward, steps_inc, prev, good_above, tol):
    return reward > good_above and steps == steps_inc and abs(prev - reward) <= tol


def candidate_order(rconc, strategy):
    """stable by |Q|: ascending (strategy 1, the first minimum :268) or descending (2, the first maximum :286)"""
    return [int(c) for c in np.argsort(np.abs(rconc) if strategy == 1 else -np.abs(rconc), kind="stable")]


class Outcome:
    """kept: surviving original indices; per_start[k] = (used, steps_incremental, baseline_reward, reward), steps_incremental -1 for
    a start that takes no part; rounds / rollouts as frirl_hip_reduce_result counts them (tree_walk only)"""

    def __init__(self, kept, per_start, rounds=None, rollouts=None):
        self.kept, self.per_start, self.rounds, self.rollouts = kept, per_start, rounds, rollouts

    @property
    def used(self):
        return [k for k, p in enumerate(self.per_start) if p[0]]

    def first(self):
        """(steps_incremental, reward) of frirl_hip_reduce_result: the first used start, start 0 where none is used"""
        p = self.per_start[self.used[0] if self.used else 0]
        return p[1], p[3]


def baseline(rp, starts, count, drop_bad_starts):
    R0 = rp.t.R0
    alive = list(range(R0))
    base = [rp.replay(alive, starts[k]) for k in range(count)]
    used = [k for k in range(count) if not drop_bad_starts or base[k][1] > rp.good_above]
    return alive, base, used


def finish(alive, base, used, prev, n):
    per = []
    for k in range(n):
        if k < len(base):
            per.append((1 if k in used else 0, base[k][0], base[k][1], prev[k]))
        else:
            per.append((0, -1, 0.0, 0.0))
    return alive, per


def sequential(trained, starts, strategy, tol=0.0, count=None, drop_bad_starts=False):
    """The reference's loop, one candidate per trial, every trial replayed from every used start."""
    rp = Replayer(trained)
    n = len(starts)
    count = n if count is None else min(max(count, 1), n)
    alive, base, used = baseline(rp, starts, count, drop_bad_starts)
    prev = [b[1] for b in base]
    if used:
        for c in candidate_order(trained.rconc, strategy):
            trial = [r for r in alive if r != c]
            out = {k: rp.replay(trial, starts[k]) for k in used}
            if all(accept(out[k][0], out[k][1], base[k][0], prev[k], rp.good_above, tol) for k in used):
                alive = trial
                for k in used:
                    prev[k] = out[k][1]
    rp.done()
    kept, per = finish(alive, base, used, prev, n)
    return Outcome(kept, per)


def walk(d, K, steps, reward, steps_inc, prev, good_above, tol):
    """The walk over nodes x starts, restated independently of csrc/reduce_walk.h: steps / reward [2^d - 1][K], node (k, bits) =
    2^k - 1 + bits; returns (bits, prev after the walk)."""
    prev = list(prev)
    bits = 0
    for k in range(d):
        node = (1 << k) - 1 + bits
        if all(accept(steps[node][i], reward[node][i], steps_inc[i], prev[i], good_above, tol) for i in range(K)):
            bits |= 1 << k
            prev = [reward[node][i] for i in range(K)]
    return bits, prev


def tree_walk(trained, starts, strategy, depth, tol=0.0, count=None, drop_bad_starts=False):
    """Rounds of min(depth, candidates left) candidates: every node of the accept/reject tree replayed from every used start."""
    rp = Replayer(trained)
    n = len(starts)
    count = n if count is None else min(max(count, 1), n)
    alive, base, used = baseline(rp, starts, count, drop_bad_starts)
    prev = [b[1] for b in base]
    K = len(used)
    order = candidate_order(trained.rconc, strategy)
    rounds, rollouts, j = 0, count, 0
    while K and j < len(order):
        d = min(depth, len(order) - j)
        cands = order[j:j + d]
        nodes = (1 << d) - 1
        steps = [[0] * K for _ in range(nodes)]
        reward = [[0.0] * K for _ in range(nodes)]
        for k in range(d):
            for bits in range(1 << k):
                gone = {cands[i] for i in range(k) if (bits >> i) & 1} | {cands[k]}
                trial = [r for r in alive if r not in gone]
                for i, s in enumerate(used):
                    steps[(1 << k) - 1 + bits][i], reward[(1 << k) - 1 + bits][i] = rp.replay(trial, starts[s])
        bits, new_prev = walk(d, K, steps, reward, [base[s][0] for s in used], [prev[s] for s in used], rp.good_above, tol)
        for i, s in enumerate(used):
            prev[s] = new_prev[i]
        gone = {cands[i] for i in range(d) if (bits >> i) & 1}
        alive = [r for r in alive if r not in gone]
        rounds += 1
        rollouts += nodes * K
        j += d
    rp.done()
    kept, per = finish(alive, base, used, prev, n)
    return Outcome(kept, per, rounds, rollouts)


def counters(R0, depth, count, K):
    """(rounds, rollouts) of frirl_hip_reduce_result for an agent with R0 rules, `count` participating and K used starts"""
    if K == 0:
        return 0, count
    rounds, rollouts, j = 0, count, 0
    while j < R0:
        d = min(depth, R0 - j)
        rounds += 1
        rollouts += ((1 << d) - 1) * K
        j += d
    return rounds, rollouts
