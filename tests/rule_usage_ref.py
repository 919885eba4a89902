"""CPU reference of the rule usage on the policy map, of the stable candidate order and of the map-validated reduction over several
caller orders (frirl_hip_rule_usage, frirl_hip_rule_order, frirl_hip_reduce_batch_map_orders) over the oracle, built from
the pieces of tests/policy_map_ref.py: every greedy action is the oracle's Five.best_action, every weight the oracle's
Five.vag_concl_weight (orc_vag_concl_weight = FIVEVagConclWeight.c), every removal five_remove_rule's; no arithmetic is restated."""
import numpy as np

from tests import policy_map_ref as pm


def action_raw(five, ave_value):
    """the value of the action universe whose VE value is `ave_value`: Five.vag_concl_weight snaps raw antecedents itself"""
    k = five.nant - 1
    idx = np.nonzero(np.asarray(five.ve)[k] == ave_value)[0]
    assert len(idx), "an action VE value that is not in the action universe's table"
    return float(np.asarray(five.u)[k][idx[0]])


def usage(five, points, action_ve, diag=None, resnapped=False):
    """(sum [R], peak [R], best [n]) of one rule base at `points` [n][nant-1] in list order: per point the oracle's greedy action, then
    the oracle's normalised Shepard weights at (point, that action): one-hot on a returned hit index, else five.weights[:R].
    Five.vag_concl_weight takes UNIVERSE values and snaps them itself, so it is asked at the point as given and the action's universe
    value: the VE point the map evaluates.
    resnapped: the antecedents handed over are the snapped VE values [snapped point, ave[best]] instead, which the oracle snaps a second
    time as if they were universe values.  That is NOT the usage of the rule base at the point; it is kept because the candidate orders
    recorded with tests/test_hip_reduce_orders.py (rule counts and margins) were drawn this way: there an order is only an input."""
    R = five.R
    total, peak, best = np.zeros(R), np.zeros(R), []
    for pt in points:
        b, _ = pm.evaluate(five, pt, action_ve, diag)
        if resnapped:
            x = np.append(pm.snapped(five, pt), action_ve[b])
        else:
            x = np.append(np.asarray(pt, dtype=np.float64), action_raw(five, action_ve[b]))
        h = five.vag_concl_weight(x)
        if h >= 0:
            w = np.zeros(R)
            w[h] = 1.0
        else:
            w = np.array(five.weights[:R])
        total = total + w                                              # ascending j, plain adds
        peak = np.maximum(peak, w)
        best.append(b)
    return total, peak, np.array(best, dtype=np.int32)


def stable_order(keys, descending=False):
    """rank(r) = #{q : key_q before key_r} + #{q < r : key_q == key_r}; NaN keys after every number, stable among themselves"""
    keys = np.asarray(keys, dtype=np.float64)

    def k(r):
        v = keys[r]
        return (1, 0.0) if np.isnan(v) else (0, -v if descending else v)
    return sorted(range(len(keys)), key=k)                             # Python's sort is stable


def reduce_map_order(u, ve, rant, rconc, points, action_ve, order, p=0, diag=None):
    """policy_map_ref.reduce_map with the caller's candidate order (a permutation of 0..R-1)"""
    R = len(rconc)
    assert sorted(order) == list(range(R))
    kept = list(range(R))
    if len(points) == 0 or R < 2:
        return pm.Outcome(kept, np.zeros(0, dtype=np.int32), 0)
    best0, _ = pm.policy_map(pm.make_five(u, ve, rant, rconc, p), points, action_ve, diag)
    tries = 0
    for c in order:
        if len(kept) == 1:
            break
        trial = [r for r in kept if r != c]
        five = pm.make_five(u, ve, rant[kept], rconc[kept], p)
        five.remove_rule(kept.index(c))
        assert five.R == len(trial)
        tries += 1
        if all(pm.evaluate(five, pt, action_ve, diag)[0] == best0[i] for i, pt in enumerate(points)):
            kept = trial
    return pm.Outcome(kept, best0, tries)


def reduce_map_orders(u, ve, rant, rconc, points, action_ve, orders, p=0, diag=None):
    """every order on its own; the one that keeps the fewest rules is chosen, ties to the lowest k.  Returns (chosen k or -1 for an
    untouched rule base, the chosen Outcome, rules kept per order)."""
    outs = [reduce_map_order(u, ve, rant, rconc, points, action_ve, o, p, diag) for o in orders]
    after = [len(o.kept) for o in outs]
    if len(points) == 0 or len(rconc) < 2:
        return -1, outs[0], after
    k = int(np.argmin(after))                                          # the first minimum
    return k, outs[k], after


def usage_order(u, ve, rant, rconc, points, action_ve, p=0, descending=False, diag=None, resnapped=False):
    """least-used first (or most-used first): the stable order of the usage sums of the un-reduced rule base; also returns the sums"""
    total, _, _ = usage(pm.make_five(u, ve, rant, rconc, p), points, action_ve, diag, resnapped)
    return stable_order(total, descending), total
