"""The packed index mirror of the rule-distance scan (five_hip_rule_distance_packed, frirl_hip_pack_indices): 6-bit universe
indices, five per 32-bit word, pidx[e][w][r].  Distances bit-identical and the same exact-hit indices as the 16-bit mirror
(option rd_packed = 0), the f64 columns and the oracle; the mirror Problem owns is repacked whenever uidx may have changed."""
import numpy as np
import pytest
import torch

import frirl_amd
from tests.problems import Batch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def np_pack(uidx, W):
    """numpy restatement of the layout: field k in word k // 5 at shift 6 * (k % 5), every column."""
    E, nant, maxR = uidx.shape
    u = uidx.astype(np.int64) & 63
    out = np.zeros((E, W, maxR), dtype=np.int64)
    for k in range(nant):
        out[:, k // 5] |= u[:, k] << (6 * (k % 5))
    return out.astype(np.uint32)


@pytest.mark.parametrize("nant", list(range(1, 17)))
def test_packed_words_by_shape(nant):
    lib = frirl_amd.lib()
    for U in (2, 41, 63, 64, 65, 101):
        W = lib.five_hip_rule_distance_packed_words(nant, U)
        served = U <= 64 and nant * U * 8 <= 4096
        assert W == ((nant + 4) // 5 if served else 0), (nant, U, W)
    assert lib.five_hip_rule_distance_packed_words(0, 41) == 0 and lib.five_hip_rule_distance_packed_words(17, 41) == 0


def scan(prob, x, materialise=True):
    d, hit = prob.rule_distance(x, materialise=materialise)
    torch.cuda.synchronize()
    return (d.cpu().numpy() if materialise else None), hit.cpu().numpy().astype(np.int64)


def plain(prob):
    return frirl_amd.Problem(prob.u, prob.ve, prob.rb, prob.nrules)      # no index mirror: the f64 columns


def assert_same(prob, nrules, d, hit, d_ref, hit_ref, what):
    assert (hit == hit_ref).all(), (what, hit, hit_ref)
    for e in range(len(nrules)):
        n = int(nrules[e])
        assert (bits(d[e, :n]) == bits(d_ref[e, :n])).all(), (what, e)


@pytest.mark.gpu
def test_pidx_is_the_packing_of_uidx():
    b = Batch(7, 41, 1001, 5, A=3, seed=3, ragged=True, maxR=1100)
    prob = b.to_device(compressed=True)
    W = frirl_amd.lib().five_hip_rule_distance_packed_words(7, 41)
    assert W == 2 and prob.pidx is not None and tuple(prob.pidx.shape) == (5, 2, 1100)
    torch.cuda.synchronize()
    want = np_pack(prob.uidx.cpu().numpy().view(np.uint16), W)
    assert (prob.pidx.cpu().numpy().view(np.uint32) == want).all()


SHAPES = [(nant, U) for nant in range(1, 7) for U in (2, 41, 63, 64, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("nant,U", SHAPES)
def test_packed_scan_bit_identical(nant, U, hip_option):
    """Ragged rule bases (odd counts, 7 rules, an empty one), nrules < maxR, R not a multiple of the 2048-rule chunk; a hit at the
    last rule of environment 0, hits in later chunks, and duplicate zero-distance rules (the lowest index wins)."""
    R, E = 4099, 6
    b = Batch(nant, U, R, E, A=0, seed=40 + nant * 7 + U, ragged=True, maxR=R + 61)
    # environment 3: rules 2500 and 3001 are copies of rule 4000 -> a query at rule 4000 hits 2500 (a later chunk, the lowest copy)
    e = 3
    n3 = int(b.nrules[e])
    src, dups = min(4000, n3 - 1), [r for r in (2500, 3001) if r < n3 - 1]
    for r in dups:
        b.uidx[e, :, r] = b.uidx[e, :, src]
        b.rb[e, :nant, r] = b.rb[e, :nant, src]
    x = b.queries(seed=U + nant, hit_fraction=0.5)
    x[e] = b.u[np.arange(nant), b.uidx[e, :, src]]
    # environment 4: a hit in the third chunk
    r4 = min(4500, int(b.nrules[4]) - 1)
    x[4] = b.u[np.arange(nant), b.uidx[4, :, r4]]
    d_ref, hit_ref = b.oracle_rule_distance(x)
    assert hit_ref[e] >= 0 and (not dups or hit_ref[e] <= min(dups))
    prob = b.to_device(compressed=True)
    assert (prob.pidx is not None) == (U <= 64)
    xd = torch.from_numpy(x).cuda()
    d, hit = scan(prob, xd)
    assert_same(prob, b.nrules, d, hit, d_ref, hit_ref, "packed vs oracle")
    _, hit0 = scan(prob, xd, materialise=False)
    assert (hit0 == hit).all(), "NULL ruledists"
    hip_option("rd_packed", 0)
    d16, hit16 = scan(prob, xd)
    assert_same(prob, b.nrules, d, hit, d16, hit16, "packed vs 16-bit mirror")
    hip_option("rd_packed", 1)
    df, hitf = scan(plain(prob), xd)
    assert_same(prob, b.nrules, d, hit, df, hitf, "packed vs f64 columns")


def check_vs_f64(prob, x, what):
    assert prob.pidx is not None
    d, hit = scan(prob, x)
    df, hitf = scan(plain(prob), x)
    assert_same(prob, prob.nrules.cpu().numpy(), d, hit, df, hitf, what)
    return hit


def query_rule(prob, e_rule):
    """x[e] = the antecedents of rule e_rule[e] of environment e (read from the 16-bit mirror)."""
    E = prob.E
    r = torch.as_tensor(e_rule, device=prob.uidx.device).long()
    idx = prob.uidx[torch.arange(E, device=r.device), :, r].long()          # [E][nant]
    return torch.stack([prob.u[k][idx[:, k]] for k in range(prob.nant)], dim=1).contiguous()


@pytest.mark.gpu
def test_inplace_uidx_edit_repacks():
    b = Batch(5, 41, 3000, 4, A=3, seed=9, ragged=False, maxR=3000)
    prob = b.to_device(compressed=True)
    x = query_rule(prob, [2999, 100, 2048, 7])
    check_vs_f64(prob, x, "before")
    # move rule 1500 of every environment onto the query point: the lowest exact hit becomes 1500 (env 1: 100 stays)
    for k in range(prob.nant):
        idx = prob.uidx[torch.arange(4, device="cuda"), k, torch.tensor([2999, 100, 2048, 7], device="cuda")]
        prob.uidx[:, k, 1500] = idx
        prob.rb[:, k, 1500] = prob.ve[k][idx.long()]
    hit = check_vs_f64(prob, x, "after an in-place edit of uidx")
    assert hit[0] <= 1500 and hit[2] <= 1500 and hit[1] <= 100 and hit[3] <= 7


@pytest.mark.gpu
def test_appended_and_merged_rules_are_scanned():
    dev = torch.device("cuda", 0)
    prob, agent, envs = frirl_amd.demo_batch("mountaincar", 8, 64, 512, dev, seed=5)
    x = query_rule(prob, [63] * 8)
    check_vs_f64(prob, x, "fresh")
    # fused episode steps append rules through prob.bases
    R0 = prob.nrules.clone()
    frirl_amd.episode_begin(prob, agent, envs)
    frirl_amd.episode_steps(prob, agent, envs, 40)
    torch.cuda.synchronize()
    assert (prob.nrules > R0).any(), "the episode steps appended no rule"
    last = (prob.nrules - 1).tolist()
    hit = check_vs_f64(prob, query_rule(prob, last), "after episode_steps")
    assert (hit >= 0).all()
    # five_hip_add_rule: one rule per environment at an off-grid point of the universes
    rng = np.random.default_rng(1)
    u = prob.u.cpu().numpy()
    pts = np.stack([u[k, rng.integers(0, prob.U, 8)] for k in range(prob.nant)], 1)
    prob.add_rule(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.full((8,), 3.0, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    hit = check_vs_f64(prob, torch.from_numpy(np.ascontiguousarray(pts)).to(dev), "after add_rule")
    assert (hit >= 0).all()
    # frirl_hip_merge_rb: sender rules taken over by every rule base
    S = 12
    snd = np.stack([u[k, rng.integers(0, prob.U, S)] for k in range(prob.nant)], 1)
    weights = torch.zeros((prob.E, prob.maxR), dtype=torch.float64, device=dev)
    n_before = prob.nrules.clone()
    prob.merge_rb(agent, torch.from_numpy(np.ascontiguousarray(snd)).to(dev), torch.linspace(-5, 5, S, dtype=torch.float64, device=dev), weights)
    torch.cuda.synchronize()
    assert (prob.nrules > n_before).any(), "the merge appended no rule"
    last = (prob.nrules - 1).tolist()
    check_vs_f64(prob, query_rule(prob, last), "after merge_rb")
