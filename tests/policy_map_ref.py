"""CPU reference of the policy map and of the reduction validated on it (frirl_hip_policy_map, frirl_hip_reduce_batch_map,
frirl_hip_log_points; DESIGN "Reduction that preserves the greedy policy on visited states") over the oracle.

Every greedy action comes from the oracle's Five.best_action (orc_five_best_action: the points snapped as its `states`, first exact
hit else Shepard, first maximum) on a rule base that holds exactly the rules of the trial, built by removing rules from a copy with
five_remove_rule's order-preserving shift: no removal arithmetic is restated here.

Diagnostics over every (trial, point) evaluation: the smallest relative gap between the two best conclusions, and the number of
bit-equal ties between the best two that are not both exact hits.  A device decision can differ from the reference's only where the
two best conclusions are closer than the device / oracle agreement on Q (tests/test_hip_q.py)."""
import numpy as np

from oracle import binding as ob


class Diag:
    def __init__(self):
        self.min_rel_gap, self.ties, self.evaluations = np.inf, 0, 0

    def note(self, conc, hits):
        """conc [A] of one evaluation, hits [A] bool: whether each conclusion is an exact hit"""
        self.evaluations += 1
        if len(conc) < 2:
            return
        order = np.argsort(-conc, kind="stable")
        a, b = int(order[0]), int(order[1])
        if conc[a] == conc[b]:
            if not (hits[a] and hits[b]):
                self.ties += 1
            return                                        # two exact hits on equal consequents: equal on the device too
        scale = max(abs(conc[a]), abs(conc[b]))
        self.min_rel_gap = min(self.min_rel_gap, (conc[a] - conc[b]) / scale)


def make_five(u, ve, rant, rconc, p=0, maxR=None):
    """an oracle rule base with the rules rant [R][nant] / rconc [R] in this order"""
    nant, U = u.shape
    return ob.Five(np.ascontiguousarray(u).ravel(), np.ascontiguousarray(ve).ravel(), nant, U, maxR or len(rconc) + 2, rant, rconc, p=p)


def snapped(five, point):
    """the VE point the oracle evaluates for `point` (orc_snap on every state universe)"""
    L, U = ob.lib(), five.U
    u, ve = five.u, five.ve
    return np.array([ve[k, L.orc_snap(ob.dp(np.ascontiguousarray(u[k])), U, float(point[k]), float(five.c.udivs[k]))] for k in range(five.nant - 1)])


def exact_hits(five, point, action_ve):
    """[A] bool: does a rule of `five` sit exactly at (snapped point, action a)?"""
    R, ns = five.R, five.nant - 1
    q = snapped(five, point)
    at_state = (five.veval[:ns, :R] == q[:, None]).all(axis=0)
    return np.array([bool((at_state & (five.veval[ns, :R] == av)).any()) for av in action_ve])


def evaluate(five, point, action_ve, diag=None):
    b, conc = five.best_action(point, action_ve)
    if diag is not None:
        diag.note(conc, exact_hits(five, point, action_ve))
    return b, conc


def policy_map(five, points, action_ve, diag=None):
    """(best [n] int, actconc [n][A]) of one rule base at `points` [n][nant-1]"""
    out = [evaluate(five, pt, action_ve, diag) for pt in points]
    return np.array([b for b, _ in out], dtype=np.int32).reshape(len(points)), np.array([c for _, c in out]).reshape(len(points), len(action_ve))


def candidate_order(rconc, strategy):
    """frirl_hip_reduce_batch's: stable by |Q|, ascending (strategy 1) or descending (2)"""
    return [int(c) for c in np.argsort(np.abs(rconc) if strategy == 1 else -np.abs(rconc), kind="stable")]


class Outcome:
    def __init__(self, kept, best0, tries):
        self.kept, self.best0, self.tries = kept, best0, tries


def reduce_map(u, ve, rant, rconc, points, action_ve, strategy, p=0, diag=None):
    """Try-remove validated on the map.  rant [R][nant], rconc [R]; points [n][nant-1] (n may be 0).  A candidate is removed iff the map
    of the rules still present minus the candidate equals best0 at every point; the last remaining rule is never tried.  With no
    point or one rule nothing is tried."""
    R = len(rconc)
    kept = list(range(R))
    if len(points) == 0 or R < 2:
        return Outcome(kept, np.zeros(0, dtype=np.int32), 0)
    best0, _ = policy_map(make_five(u, ve, rant, rconc, p), points, action_ve, diag)
    tries = 0
    for c in candidate_order(rconc, strategy):
        if len(kept) == 1:
            break
        trial = [r for r in kept if r != c]
        five = make_five(u, ve, rant[kept], rconc[kept], p)
        five.remove_rule(kept.index(c))                              # five_remove_rule keeps the order of the others
        assert five.R == len(trial)
        tries += 1
        # points in order up to the first one whose greedy action differs: that point alone decides the rejection, whatever the
        # later ones would give, so the diagnostics cover every evaluation a decision rests on
        if all(evaluate(five, pt, action_ve, diag)[0] == best0[i] for i, pt in enumerate(points)):
            kept = trial
    return Outcome(kept, best0, tries)


def log_points(obs, q_obs, success, start, length, E, cap, only_successful=False):
    """Per agent the de-duplicated points of its logs (arrays as frirl_hip_rollout_log's, logs e * n_logs + j of agent e): a start record
    contributes obs, every other record q_obs; bit-wise comparison; first occurrence over (log ascending, record ascending) first.
    Returns (list of [count][ns] arrays cut at cap, overflow [E])."""
    Q, T, ns = obs.shape
    n_logs = Q // E
    out, overflow = [], np.zeros(E, dtype=np.int32)
    for e in range(E):
        seen, pts = set(), []
        for j in range(n_logs):
            q = e * n_logs + j
            n = min(max(int(length[q]), 0), T)
            r = 0
            while r < n:
                end = r + 1
                while end < n and not start[q, end]:
                    end += 1                                         # the episode is records [r, end)
                if not only_successful or success[q, end - 1] == 1:
                    for i in range(r, end):
                        x = obs[q, i] if start[q, i] else q_obs[q, i]
                        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
                        if key not in seen:
                            seen.add(key)
                            pts.append(np.array(x, dtype=np.float64))
                r = end
        overflow[e] = 1 if len(pts) > cap else 0
        out.append(np.array(pts[:cap]).reshape(-1, ns))
    return out, overflow


def episode_points(fr, start, max_steps=1000):
    """The observations the greedy policy of the oracle agent `fr` is asked at in one episode from `start`: the un-quantised start,
    then every step's quantised observation, the terminal one included -- what frirl_hip_rollout_record logs as obs of the start record
    and q_obs of every other record.  Not de-duplicated."""
    actions = fr.dim(fr.nant - 1)["values"]
    x = np.array(start, dtype=np.float64)
    obs, pts = x, [x.copy()]
    for _ in range(max_steps):
        a = fr.get_best_action(obs)
        x, _, success, q = fr.env_step(actions[a], x)
        pts.append(q.copy())
        obs = q
        if success == 1:
            break
    return np.array(pts)


def dedup(points):
    """first occurrences, bit-wise, in order"""
    seen, out = set(), []
    for x in points:
        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
        if key not in seen:
            seen.add(key)
            out.append(x)
    return np.array(out).reshape(-1, points.shape[1])
