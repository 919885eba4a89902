"""numpy restatements of the selection contract of include/frirl_hip.h (frirl_hip_clone_agents, frirl_hip_select_plan), written from
the contract, not from the C code.  No GPU needed."""
import numpy as np

KEPT, CLONED, BAD_SRC, CHAINED, BAD_RULES = range(5)

# what a clone takes from its source, row arrays ([E][rows][maxR] or [E][maxR]) and per-agent scalars ([E] or [E][nant])
ROW_ARRAYS = ("rb", "rant", "uidx", "weights")
SCALARS = ("fus", "spread_ant", "spread_R")
# what it keeps
KEPT_ARRAYS = ("start_states", "episode", "states", "q_ant", "done", "ep_steps", "ep_reward", "status", "episodes")


def clone_status(src, nrules, maxR):
    E = len(src)
    st = np.zeros(E, dtype=np.int32)
    for e in range(E):
        s = int(src[e])
        if s == e:
            st[e] = KEPT
        elif s < 0 or s >= E:
            st[e] = BAD_SRC
        elif int(src[s]) != s:
            st[e] = CHAINED
        elif not 1 <= int(nrules[s]) <= maxR:
            st[e] = BAD_RULES
        else:
            st[e] = CLONED
    return st


def _bound(n, maxR):
    return maxR if (n < 0 or n > maxR) else n


def clone_ref(state, src):
    """state: dict of numpy arrays named as the fields of frirl_hip_rulebases / _envs / _convergence plus `weights` (a missing or None
    entry = the NULL pointer).  Returns (the state after frirl_hip_clone_agents(src), status [E]); the input is not modified."""
    out = {k: (None if v is None else np.array(v, copy=True)) for k, v in state.items()}
    rb, nrules = state["rb"], state["nrules"]
    maxR = rb.shape[2]
    st = clone_status(src, nrules, maxR)
    for e in np.nonzero(st == CLONED)[0]:
        s = int(src[e])
        ns = int(nrules[s])
        cols = max(_bound(int(nrules[e]), maxR), ns)
        for k in ROW_ARRAYS:
            if state.get(k) is None:
                continue
            row = np.zeros_like(state[k][s])
            row[..., :ns] = state[k][s][..., :ns]
            out[k][e][..., :cols] = row[..., :cols]
        out["nrules"][e] = ns
        for k in SCALARS:
            if state.get(k) is not None:
                out[k][e] = state[k][s]
        if state.get("prev_rconc") is not None:
            colsp = max(cols, _bound(int(state["prev_nrules"][e]), maxR))
            row = np.zeros(maxR)
            row[:ns] = rb[s][-1][:ns]
            out["prev_rconc"][e][:colsp] = row[:colsp]
            out["prev_nrules"][e] = ns
            out["prev_steps"][e] = -1
            out["prev_reward"][e] = -1.0
            out["converged"][e] = 0
            if state.get("epended") is not None:
                out["epended"][e] = 0
    return out, st


def plan_ref(scores, parents, replace, eligible=None):
    """scores: sequence of (successes, reward_sum).  Returns (src [E], rank [N]) of frirl_hip_select_plan; ValueError where it refuses."""
    E = len(scores)
    if E < 1 or parents < 1 or replace < 0:
        raise ValueError("sizes")
    who = [e for e in range(E) if eligible is None or eligible[e]]
    for e in who:
        if scores[e][1] != scores[e][1]:
            raise ValueError(f"agent {e}: NaN")
    if parents + replace > len(who):
        raise ValueError("parents + replace > N")
    rank = sorted(who, key=lambda e: (-scores[e][0], -scores[e][1], e))
    src = list(range(E))
    for k in range(replace):
        src[rank[len(rank) - 1 - k]] = rank[k % parents]
    return np.array(src, dtype=np.int32), np.array(rank, dtype=np.int32)
