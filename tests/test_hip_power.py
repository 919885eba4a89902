"""Shepard powers other than nant on the GPU, against the oracle.

Every entry point that takes a power runs other kernels at p != nant than at the default (run-time weight forms, kernel variants
without rule slices; csrc/sweeps.h).  The rest of the suite runs at p = 0; here

 * the weight forms themselves are probed (five_hip_shepard_weight_check) against s^(-p/2) from `decimal` at 60 digits, bound
   p x 4e-16 (tests/shepard_ref.py; the same bound holds for the oracle's chain on the CPU, tests/test_oracle_golden.py);
 * the entry points run at p in {1, 2, nant + 1} and at 3 / 5 where that differs from nant (the PowU shortcuts), against an
   oracle rule base built with the same power (ob.Five(..., p=p)).  One explicit p = nant call per group equals p = 0 bit for bit.

Bars are those the same entry points have at p = nant: hit indices, exact-hit conclusions, appended antecedents and rule counts exact;
interpolated values 1e-11 (tree sums), 1e-10 (sequential sums on synthetic shared bases), 1e-9 after SARSA rounds.  Arg-max picks are
compared unless the oracle's two best conclusions lie within 1e-9 relative; every test asserts that at most 10 % of its picks are
skipped that way (the counts for the seeds used are in the docstrings: they depend on the oracle alone).
Measured figures: profiles/r08_shepard_power.md."""
import ctypes as C

import numpy as np
import pytest

import frirl_amd
from oracle import binding as ob
from tests import shepard_ref as sr
from tests.problems import Batch, demo_device_batch, device_agent

pytestmark = pytest.mark.gpu
RTOL = 1e-11            # tree sums (tests/test_hip_q.py)
RTOL_SHARED = 1e-10     # sequential sums on synthetic shared bases (tests/test_hip_q.py)
TIE = 1e-9
DP = C.POINTER(C.c_double)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dp(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(DP)


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def powers(nant):
    """1, 2, nant + 1, and 3 / 5 where they differ from nant."""
    return sorted({1, 2, nant + 1, 3, 5} - {nant})


def clear_max(ac):
    """The oracle's maximum is clear: its two best conclusions are more than 1e-9 relative apart."""
    srt = np.sort(ac)
    return len(srt) < 2 or (srt[-1] - srt[-2]) > TIE * max(1.0, abs(srt[-1]))


def same_bits(a, b):
    """Two device tensors of doubles hold the same bits (NaN included)."""
    import torch
    return bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())


# ---- the weight forms ------------------------------------------------------------------------------------------------------------
def weight_check(s, p, form):
    import torch
    w = torch.full_like(s, float("nan"))
    rc = frirl_amd.lib().five_hip_shepard_weight_check(C.c_void_p(s.data_ptr()), s.numel(), p, form, C.c_void_p(w.data_ptr()), None)
    frirl_amd.check(rc, "five_hip_shepard_weight_check")
    torch.cuda.synchronize()
    return w.cpu().numpy()


@pytest.mark.parametrize("p", sr.POWERS)
def test_weight_forms_meet_the_derived_bound(p):
    """shepard_w in its four forms (0: run-time loop, 1: PowU, 2: PowC<p>, 3: pinned PowC<p>) against s^(-p/2) at 60 digits on the
    ~20 000 inputs of tests/shepard_ref.py: relative error <= p x 4e-16 for every form; forms 0 and 1 (one source) within the same
    bound of each other; the pinned series is the series bit for bit.  Measured maxima: profiles/r08_shepard_power.md."""
    s = dev(np.array(sr.inputs()))          # a writable copy: the shared input array is read-only
    keep = sr.exact()[p][2]
    w = [weight_check(s, p, form) for form in range(4)]
    for form in range(4):
        err, i = sr.rel_error(w[form], p)
        print(f"shepard_weight p={p} form={form} max_rel_err={err:.3e} at s={float(sr.inputs()[i]):.17g}")
    for form in range(4):
        assert np.isfinite(w[form][keep]).all() and (w[form][keep] > 0).all(), form
        err, i = sr.rel_error(w[form], p)
        assert err <= sr.bound(p), (form, p, err, float(sr.inputs()[i]))
    assert rel(w[1][keep], w[0][keep]).max() <= sr.bound(p)
    assert (w[2][keep] == w[3][keep]).all(), "pinning the coefficients in registers changes no bit"


def test_weight_probe_lengths():
    """n = 0 launches nothing; a length that is no multiple of the block writes exactly n values."""
    import torch
    assert frirl_amd.lib().five_hip_shepard_weight_check(None, 0, 3, 0, None, None) == 0
    s = dev(np.array(sr.inputs()[:300]))
    w = torch.full((301,), -1.0, dtype=torch.float64, device="cuda")
    frirl_amd.check(frirl_amd.lib().five_hip_shepard_weight_check(C.c_void_p(s.data_ptr()), 257, 5, 2, C.c_void_p(w.data_ptr()), None), "probe")
    torch.cuda.synchronize()
    w = w.cpu().numpy()
    assert (w[:257] > 0).all() and (w[257:] == -1.0).all()


# ---- per-environment Q kernels -----------------------------------------------------------------------------------------------------
def q_case(nant, U, R, E, A, seed):
    """Ragged rule bases: environment 0 full (its last rule is hit), 1 a one-rule base, 2 an odd count (a prefix of environment 3's
    rules: Batch leaves environment 2 empty), the rest random."""
    b = Batch(nant, U, R, E, A=A, seed=seed, ragged=True)
    b.nrules[1] = 1
    n2 = int(b.nrules[3]) - 1
    b.nrules[2] = n2 if n2 % 2 else n2 - 1
    b.rb[2], b.uidx[2] = b.rb[3], b.uidx[3]
    assert b.nrules[2] % 2 == 1 and b.nrules[2] >= 3 and (b.nrules > 0).all()
    x = b.queries(seed=seed + 1, hit_fraction=0.4)
    return b, x


def check_q(b, x, p, conc, hit, w, hitw, envs):
    nh = 0
    for e in envs:
        f = b.five(e, p)
        assert f.c.p == p
        n = f.R
        h, c = f.vag_concl(x[e])
        assert hit[e] == h and hitw[e] == h, e
        if h >= 0:
            nh += 1
            assert c == conc[e], "exact hit returns the rule's consequent bit for bit"
            assert np.isnan(w[e]).all(), "weights row of an exact-hit environment must stay untouched"
        else:
            assert rel(conc[e], c) <= RTOL, (e, p, conc[e], c)
            assert f.vag_concl_weight(x[e]) == -1
            assert rel(w[e, :n], f.weights[:n]).max() <= RTOL, (e, p)
            assert abs(w[e, :n].sum() - 1.0) < 1e-12
    return nh


def longdouble_bar(f, xa, p, oracle_value):
    """The bar for an interpolated value that misses RTOL: the same Shepard sums in numpy.longdouble from the oracle's distances, the
    oracle's own deviation from them, times 8 (the kernels' summation order differs from the oracle's and both are double), at most 1e-9."""
    assert f.rule_distance(xa) == -1
    n = f.R
    d = np.array(f.ruledists[:n], dtype=np.longdouble)
    w = 1 / d ** p
    ld = (w * np.array(f.rconc[:n], dtype=np.longdouble)).sum() / w.sum()
    return min(1e-9, 8 * float(abs(oracle_value - ld) / abs(ld)))


ONE_RULE_BASE = 1      # q_case: this environment has a single rule


def check_gba(b, states, ave, avals, p, actconc, best, envs):
    """Returns (picks compared with the oracle's, picks skipped as near-ties of the oracle) over the pick set: `envs` without the
    one-rule base, which concludes its one consequent for every action (a tie in real arithmetic, by construction) and so has no pick;
    its conclusions are checked like all others.  Every pick, of the one-rule base too, must be the first maximum of the device's own
    conclusions.  Conclusions of actions that hit a rule exactly are the rule's
    consequent bit for bit; interpolated ones meet RTOL or, where consequents of both signs cancel, longdouble_bar."""
    done = skipped = 0
    for e in envs:
        f = b.five(e, p)
        bo, ac = f.best_action(states[e], ave)
        n = int(b.nrules[e])
        for a in range(len(ave)):
            xa = np.concatenate([states[e], [avals[a]]])
            if f.vag_concl(xa)[0] >= 0:
                assert actconc[e, a] == ac[a], (e, p, a, "exact hit: the consequent bit for bit")
            elif rel(actconc[e, a], ac[a]) > RTOL:
                bar = longdouble_bar(f, xa, p, ac[a])
                print(f"get_best_action e={e} a={a} p={p}: device {actconc[e, a]!r} oracle {ac[a]!r} rel {rel(actconc[e, a], ac[a]):.3e} "
                      f"> {RTOL:g}; bar from the long-double sums {bar:.3e}")
                assert rel(actconc[e, a], ac[a]) <= bar, (e, p, a, actconc[e, a], ac[a], bar)
        assert best[e] == int(np.argmax(actconc[e])), (e, p, actconc[e])
        if e == ONE_RULE_BASE:
            assert n == 1
            continue
        if clear_max(ac):
            done += 1
            assert best[e] == bo, (e, p, actconc[e], ac)
        else:
            skipped += 1
            assert abs(ac[best[e]] - np.sort(ac)[-1]) <= TIE * max(1.0, abs(np.sort(ac)[-1]))
    return done, skipped


SMALL_E = [(3, 41, 33, 6, 3), (5, 41, 367, 6, 3), (5, 41, 4097, 6, 3)]


@pytest.mark.parametrize("nant,U,R,E,A,p", [c + (p,) for c in SMALL_E for p in powers(c[0])])
def test_q_kernels_few_environments(nant, U, R, E, A, p):
    """vag_concl, vag_concl_weight, get_best_action with E < 256 (1024-thread kernels, run-time loop form) against b.five(e, p); R = 4097
    leaves an odd tail beyond two sweeps.  Near-ties of the oracle: 0 of 5 picks in every case (the sixth is the one-rule base)."""
    import torch
    b, x = q_case(nant, U, R, E, A, seed=300 + R)
    ave, avals = b.action_ve()
    states = np.ascontiguousarray(x[:, : nant - 1])
    prob = b.to_device()
    conc, hit = prob.vag_concl(dev(x), p=p)
    w, hitw = prob.vag_concl_weight(dev(x), p=p)
    actconc, best = prob.get_best_action(dev(states), dev(ave), p=p)
    torch.cuda.synchronize()
    nh = check_q(b, x, p, conc.cpu().numpy(), hit.cpu().numpy(), w.cpu().numpy(), hitw.cpu().numpy(), range(E))
    assert 0 < nh < E and hit.cpu().numpy()[0] == R - 1, "hits, misses, and a hit on the last rule"
    done, skipped = check_gba(b, states, ave, avals, p, actconc.cpu().numpy(), best.cpu().numpy(), range(E))
    assert skipped * 10 <= done + skipped, (done, skipped)


@pytest.mark.parametrize("nant,U,R,E,A", SMALL_E)
def test_q_kernels_explicit_nant_is_the_default(nant, U, R, E, A):
    """p = nant given explicitly is the p = 0 call bit for bit."""
    import torch
    b, x = q_case(nant, U, R, E, A, seed=300 + R)
    ave, _ = b.action_ve()
    states = np.ascontiguousarray(x[:, : nant - 1])
    prob = b.to_device()
    out = []
    for p in (0, nant):
        conc, hit = prob.vag_concl(dev(x), p=p)
        w, _ = prob.vag_concl_weight(dev(x), p=p, weights=torch.zeros((E, b.maxR), dtype=torch.float64, device="cuda"))
        actconc, best = prob.get_best_action(dev(states), dev(ave), p=p)
        torch.cuda.synchronize()
        out.append((conc, hit, w, actconc, best))
    for a0, a1 in zip(*out):
        assert same_bits(a0.double(), a1.double())


@pytest.mark.parametrize("p", powers(5))
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("A", [3, 8, 13, 32])
def test_q_kernels_many_environments(A, compressed, p):
    """E = 259 >= 256: the 256-thread kernels -- sweep_gba (A <= 8), sweep_gba_many (A = 13) and, through `no_many` and at A = 32,
    sweep_gba_wide -- at (5, 41, 367) with and without the index mirror.  Every 7th environment plus the one-rule and the odd base are
    compared.  Near-ties of the oracle: 0 of 38 picks for every A and p (the 39th is the one-rule base)."""
    import torch
    nant, U, R, E = 5, 41, 367, 259
    b, x = q_case(nant, U, R, E, A, seed=500 + A)
    ave, avals = b.action_ve()
    states = np.ascontiguousarray(x[:, : nant - 1])
    prob = b.to_device(compressed=compressed)
    envs = list(range(0, E, 7)) + [1, 2]
    conc, hit = prob.vag_concl(dev(x), p=p)
    w, hitw = prob.vag_concl_weight(dev(x), p=p)
    torch.cuda.synchronize()
    nh = check_q(b, x, p, conc.cpu().numpy(), hit.cpu().numpy(), w.cpu().numpy(), hitw.cpu().numpy(), envs)
    assert 0 < nh < len(envs)
    got = {}
    for nm in (0, 1):
        old = frirl_amd.set_option("no_many", nm)
        try:
            actconc, best = prob.get_best_action(dev(states), dev(ave), p=p)
            torch.cuda.synchronize()
        finally:
            frirl_amd.set_option("no_many", old)
        got[nm] = (actconc.cpu().numpy(), best.cpu().numpy())
        done, skipped = check_gba(b, states, ave, avals, p, got[nm][0], got[nm][1], envs)
        assert skipped * 10 <= done + skipped, (done, skipped)
    assert rel(got[0][0], got[1][0]).max() <= 10 * RTOL      # two summation orders (tests/test_hip_q.py)
    if p == 1:      # once per (A, compressed): explicit p = nant is the default bit for bit
        a0, b0 = prob.get_best_action(dev(states), dev(ave), p=0)
        a1, b1 = prob.get_best_action(dev(states), dev(ave), p=nant)
        c0, _ = prob.vag_concl(dev(x), p=0)
        c1, _ = prob.vag_concl(dev(x), p=nant)
        torch.cuda.synchronize()
        assert same_bits(a0, a1) and (b0 == b1).all() and same_bits(c0, c1)


# ---- shared-base query kernels ---------------------------------------------------------------------------------------------------
def shared_case(nant, U, R, A):
    f0 = ob.synth_problem(nant, U, R, A, seed=nant * 1000 + R)
    maxR = f0.maxR + (f0.maxR & 1)
    rb = np.zeros((1, nant + 1, maxR))
    rb[0, :nant, :R] = f0.veval[:, :R]
    rb[0, nant, :R] = f0.rconc[:R]
    Qn, st = 260, 99
    x = np.zeros((Qn, nant))
    for i in range(Qn):
        x[i], st = ob.synth_query(f0, st, i)
    aidx = np.linspace(0, U - 1, A).astype(int)
    ave, avals = np.array(f0.ve)[nant - 1, aidx].copy(), np.array(f0.u)[nant - 1, aidx].copy()
    return f0, rb, x, ave, avals


SHARED = [(2, 41, 300, 3), (5, 41, 367, 21), (8, 101, 1500, 5)]


@pytest.mark.parametrize("nant,U,R,A,p", [c + (p,) for c in SHARED for p in powers(c[0])])
def test_shared_base_queries(nant, U, R, A, p):
    """vag_concl_shared / get_best_action_shared (PowU form at p != nant; 3 and 5 take its shortcuts) on 260 queries, 1 in 8 an exact
    hit, against ob.synth_problem(..., p=p): hits and clear first maxima exact, conclusions 1e-10 (sequential sums).  Near-ties of the
    oracle: 0 of 260 picks for every shape and power."""
    import torch
    f0, rb, x, ave, avals = shared_case(nant, U, R, A)
    f = ob.synth_problem(nant, U, R, A, seed=nant * 1000 + R, p=p)
    assert f.c.p == p
    prob = frirl_amd.Problem(dev(np.array(f.u)), dev(np.array(f.ve)), dev(rb), dev(np.array([R], dtype=np.int32)))
    states = np.ascontiguousarray(x[:, : nant - 1])
    conc, hit = prob.vag_concl_shared(dev(x), p=p)
    actconc, best = prob.get_best_action_shared(dev(states), dev(ave), p=p)
    torch.cuda.synchronize()
    conc, hit, actconc, best = conc.cpu().numpy(), hit.cpu().numpy(), actconc.cpu().numpy(), best.cpu().numpy()
    hits = skipped = exact_actions = 0
    for i in range(len(x)):
        h, c = f.vag_concl(x[i])
        assert hit[i] == h, (i, hit[i], h)
        hits += h >= 0
        assert (conc[i] == c) if h >= 0 else (rel(conc[i], c) <= RTOL_SHARED), (i, p, conc[i], c)
        bo, ac = f.best_action(states[i], ave)
        assert rel(actconc[i], ac).max() <= RTOL_SHARED, (i, p)
        for a in range(A):
            if f.vag_concl(np.concatenate([states[i], [avals[a]]]))[0] >= 0:
                exact_actions += 1
                assert actconc[i, a] == ac[a], (i, a, p, "exact hit: the consequent bit for bit")
        if clear_max(ac):
            assert best[i] == bo, (i, p, actconc[i], ac)
        else:
            skipped += 1
    assert hits >= len(x) // 10 and skipped * 10 <= len(x), (hits, skipped)
    assert exact_actions > 0, "no action conclusion with an exact hit exercised"
    if p == 1:      # once per shape: explicit p = nant is the default bit for bit
        c0, h0 = prob.vag_concl_shared(dev(x), p=0)
        c1, h1 = prob.vag_concl_shared(dev(x), p=nant)
        a0, b0 = prob.get_best_action_shared(dev(states), dev(ave), p=0)
        a1, b1 = prob.get_best_action_shared(dev(states), dev(ave), p=nant)
        torch.cuda.synchronize()
        assert same_bits(c0, c1) and (h0 == h1).all() and same_bits(a0, a1) and (b0 == b1).all()


# ---- five_hip_bestact and the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nant,U,R,p", [(3, 41, 110, p) for p in [0] + powers(3)] + [(5, 41, 2049, p) for p in [0] + powers(5)])
def test_mirror_and_bestact(nant, U, R, p):
    """five_hip_mirror_create(..., p): vag_concl, vag_concl_weight, bestact and get_best_action of the mirror, and the batched
    five_hip_bestact on the oracle's distances, against ob.Five(..., p=p) / orc_bestact.  p = 0 runs the same checks at the default and,
    for p = nant given explicitly, the mirror returns the bits of the default.  Near-ties of the oracle: 0 of 12 picks."""
    import torch
    L = frirl_amd.lib()
    A = 3
    b = Batch(nant, U, R, 1, A=A, seed=40 + R, ragged=False)
    f = b.five(0, p)
    assert f.c.p == (p or nant)
    ave, avals = b.action_ve()
    u, ve = np.ascontiguousarray(b.u.ravel()), np.ascontiguousarray(b.ve.ravel())
    prob = b.to_device()
    mirrors = [L.five_hip_mirror_create(nant, U, dp(u), dp(ve), b.maxR, q) for q in ([p] if p else [0, nant])]
    assert all(mirrors), L.frirl_hip_last_error()
    try:
        keep = [np.ascontiguousarray(f.veval[k, :R]) for k in range(nant)]
        rows = (DP * nant)(*[dp(a) for a in keep])
        for m in mirrors:
            assert L.five_hip_mirror_upload(m, R, rows, dp(np.ascontiguousarray(f.rconc[:R]))) == 0
        rng = np.random.default_rng(1)
        hit, conc = C.c_uint32(), C.c_double()
        misses = skipped = exact_actions = 0
        for q in range(12):
            if q % 3 == 0:
                x = np.ascontiguousarray(f.rant[R - 1 if q == 0 else rng.integers(R)])
            else:
                x = np.array([rng.uniform(b.u[k, 0], b.u[k, -2]) for k in range(nant)])
            outs = []
            for m in mirrors:
                assert L.five_hip_mirror_vag_concl(m, dp(x), C.byref(conc), C.byref(hit)) == 0
                h, c = f.vag_concl(x)
                vc = conc.value
                assert (-1 if hit.value == frirl_amd.NO_HIT else hit.value) == h
                assert vc == c if h >= 0 else abs(vc - c) <= RTOL * abs(c), (q, p, vc, c)
                w = np.full(R, np.nan)
                assert L.five_hip_mirror_vag_concl_weight(m, dp(x), dp(w), C.byref(hit)) == 0
                ac = np.zeros(A)
                best = C.c_uint32()
                assert L.five_hip_mirror_get_best_action(m, dp(np.ascontiguousarray(x[: nant - 1])), dp(ave), A, dp(ac), C.byref(best)) == 0
                bo, aco = f.best_action(x[: nant - 1], ave)
                assert rel(ac, aco).max() <= RTOL, (q, p, ac, aco)
                for a in range(A):
                    if f.vag_concl(np.concatenate([x[: nant - 1], [avals[a]]]))[0] >= 0:
                        exact_actions += 1
                        assert ac[a] == aco[a], (q, a, p, "exact hit: the consequent bit for bit")
                if clear_max(aco):
                    assert best.value == bo
                else:
                    skipped += 1
                cb = np.nan
                if f.vag_concl_weight(x) == -1:
                    assert rel(w, f.weights[:R]).max() <= RTOL, (q, p)
                    f.rule_distance(x)
                    dd = np.ascontiguousarray(f.ruledists[:R])
                    ref = ob.lib().orc_bestact(f.h, dp(dd))
                    assert L.five_hip_mirror_bestact(m, dp(dd), C.byref(conc)) == 0
                    assert abs(conc.value - ref) <= RTOL * abs(ref), (q, p, conc.value, ref)
                    cb = conc.value
                    if m == mirrors[0]:
                        misses += 1
                        drow = np.zeros((1, b.maxR))
                        drow[0, :R] = dd
                        out = torch.zeros((1,), dtype=torch.float64, device="cuda")
                        frirl_amd.check(L.five_hip_bestact(C.byref(prob.bases), nant, p, C.c_void_p(dev(drow).data_ptr()), C.c_void_p(out.data_ptr()), None),
                                        "five_hip_bestact")
                        torch.cuda.synchronize()
                        assert abs(float(out[0]) - ref) <= RTOL * abs(ref), (q, p, float(out[0]), ref)
                else:
                    assert np.isnan(w).all()
                outs.append((vc, w.copy(), ac.copy(), best.value, cb))
            if len(outs) == 2:      # mirror created with p = nant against the one created with p = 0
                for a0, a1 in zip(outs[0], outs[1]):
                    assert np.array_equal(np.asarray(a0), np.asarray(a1), equal_nan=True), (q, a0, a1)
        assert misses >= 6 and skipped * 10 <= 12 * len(mirrors) and exact_actions > 0
    finally:
        for m in mirrors:
            L.five_hip_mirror_destroy(m)


# ---- frirl_hip_update_sarsa ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,episodes,p", [("mountaincar", 6, p) for p in powers(3)] + [("acrobot", 5, p) for p in powers(5)])
def test_update_sarsa_rounds(env, episodes, p):
    """The round test of tests/test_hip_sarsa.py with agent.p = p against Five.update_sarsa on ob.Five(..., p=p): rule counts, branch
    taken, sticky flag and appended antecedents exact, consequents 1e-9.  The first round is also run at p = 0 and p = nant on copies: same
    bits."""
    import torch
    E, ROUNDS = 64, 4
    b, fr = demo_device_batch(env, episodes, E)
    nant, R0 = b.nant, int(b.nrules[0])
    oag = fr.agent()
    dims = [fr.dim(k) for k in range(nant)]

    def device_side(power):
        prob = b.to_device()
        agent = device_agent(fr, p=power)
        rant0 = torch.zeros((E, nant, b.maxR), dtype=torch.float64, device="cuda")
        rant0[:, :, :R0] = dev(np.ascontiguousarray(b.rant.T))[None]
        return prob, agent, frirl_amd.Envs(prob, "cuda", rant_init=rant0)

    prob, agent, envs = device_side(p)
    assert agent.desc.p == p
    fives = [ob.Five(b.u.ravel(), b.ve.ravel(), nant, b.U, b.maxR, b.rant, np.ascontiguousarray(b.rb[e, nant, :R0]), p=p) for e in range(E)]
    fus = np.zeros(E)
    rng = np.random.default_rng(11)
    seen = set()
    for rnd in range(ROUNDS):
        q_ant, cur, reward = np.zeros((E, nant)), np.zeros((E, nant)), np.zeros(E)
        for e in range(E):
            for k in range(nant):
                v = dims[k]["values"]
                q_ant[e, k] = v[rng.integers(len(v))]
                cur[e, k] = v[rng.integers(len(v))]
            if e % 5 == 3:      # off-grid state: Shepard spread / snapped insert
                for k in range(nant - 1):
                    v = dims[k]["values"]
                    q_ant[e, k] = rng.uniform(v[0], v[-1]) * 0.9
            reward[e] = [-10.0, 1000.0, -3000.0 * rng.random(), 20 * rng.random() - 10][e % 4]
        active = np.ones(E, dtype=np.uint8)
        active[E - 1] = 0
        if rnd == 0:
            twins = [device_side(0), device_side(nant)]
            for pr, ag, en in twins:
                frirl_amd.update_sarsa(pr, ag, en, dev(q_ant), dev(reward), dev(cur), active=dev(active))
            torch.cuda.synchronize()
            assert same_bits(twins[0][0].rb, twins[1][0].rb) and (twins[0][0].nrules == twins[1][0].nrules).all()
            assert (twins[0][2].status == twins[1][2].status).all() and same_bits(twins[0][2].rant, twins[1][2].rant)
        frirl_amd.update_sarsa(prob, agent, envs, dev(q_ant), dev(reward), dev(cur), active=dev(active))
        torch.cuda.synchronize()
        nr, st, fus_d = prob.nrules.cpu().numpy(), envs.status.cpu().numpy(), envs.fus.cpu().numpy()
        rb, rant = prob.rb.cpu().numpy(), envs.rant.cpu().numpy()
        for e in range(E):
            f = fives[e]
            if not active[e]:
                assert st[e] == frirl_amd.UPD_INACTIVE and nr[e] == f.R
                continue
            Rb = f.R
            fus[e] = f.update_sarsa(oag, fus[e], q_ant[e], reward[e], cur[e])
            assert nr[e] == f.R, (rnd, e)
            assert fus_d[e] == int(fus[e]), (rnd, e)
            if f.R > Rb:
                assert st[e] == frirl_amd.UPD_INSERTED
                assert (rant[e, :, Rb] == f.rant[Rb]).all(), "appended rule antecedents (grid-snapped)"
                assert (rb[e, :nant, Rb] == f.veval[:, Rb]).all()
            else:
                assert st[e] in (frirl_amd.UPD_EXACT, frirl_amd.UPD_SPREAD, frirl_amd.UPD_SKIPPED)
            seen.add(int(st[e]))
            n = f.R
            assert (np.abs(rb[e, nant, :n] - f.rconc[:n]) / np.maximum(np.abs(f.rconc[:n]), 1e-9)).max() <= 1e-9, (rnd, e, st[e])
    assert {frirl_amd.UPD_EXACT, frirl_amd.UPD_SPREAD, frirl_amd.UPD_INSERTED} <= seen, seen


# ---- frirl_hip_weights_from_spread and frirl_hip_merge_rb ------------------------------------------------------------------------
def merge_case(nant, p, weight_thr=0.05):
    """Two synthetic receivers of about 100 rules (one odd count), a rule grid of every 4th universe point, S = 12 sender rules: ten from
    another synthetic base, two copies of receiver 0's rules (exact hits leave the weights array as it is).  No GPU needed."""
    U, R, S = 41, 100, 12
    b = Batch(nant, U, R, 2, A=3, seed=900 + nant, ragged=False, maxR=R + 16)
    b.nrules[1] = R - 1
    grids = [np.ascontiguousarray(b.u[k, ::4]) for k in range(nant)]
    snd = Batch(nant, U, S, 1, A=3, seed=950 + nant, ragged=False)
    srant = np.ascontiguousarray(snd.u[np.arange(nant)[:, None], snd.uidx[0, :, :S]].T)
    srconc = np.ascontiguousarray(snd.rb[0, nant, :S])
    for j, r in ((3, 7), (9, R - 2)):
        srant[j] = b.u[np.arange(nant), b.uidx[0, :, r]]
    hp = dict(alpha=0.5, gamma=1.0, qdiff_pos=800.0, qdiff_neg=-800.0, weight_thr=weight_thr, skip_rules=1)
    oag = ob.Agent(hp["alpha"], hp["gamma"], hp["qdiff_pos"], hp["qdiff_neg"], hp["weight_thr"], hp["skip_rules"], grids)
    rng = np.random.default_rng(nant)
    spread = np.ascontiguousarray(np.array([[rng.uniform(b.u[k, 0], b.u[k, -2]) for k in range(nant)] for _ in range(2)]))
    fives = []
    for e in range(2):
        f = b.five(e, p)
        assert f.vag_concl_weight(spread[e]) == -1          # FIVERB.weights as an interpolated SARSA update leaves it
        fives.append(f)
    return b, grids, hp, oag, srant, srconc, spread, fives


@pytest.mark.parametrize("nant", [3, 5])
def test_weights_from_spread_and_merge_rb_at_power_2(nant):
    """frirl_hip_weights_from_spread(p = 2) against FIVE_vag_concl_weight of the oracle at p = 2 (1e-11), then frirl_hip_merge_rb with
    agent.p = 2 against the oracle's merge_rb on the p = 2 rule bases, starting from those weights: rule counts, appended antecedents and
    rule order exact, consequents 1e-9 (the bar of tests/test_hip_merge.py).  The merge inserts, blends and spreads."""
    import torch
    p = 2
    b, grids, hp, oag, srant, srconc, spread, fives = merge_case(nant, p)
    E, maxR = 2, b.maxR
    prob = b.to_device(compressed=True)
    grid_div = [float(g[1] - g[0]) for g in grids]
    action_ve = b.ve[nant - 1, ::4]
    agent = frirl_amd.Agent("cuda", nant, grids, grid_div, [0.0] * nant, action_ve, hp["alpha"], hp["gamma"], hp["qdiff_pos"], hp["qdiff_neg"],
                            hp["weight_thr"], hp["skip_rules"], p, frirl_amd.ENV_EXTERNAL)
    store = torch.zeros((E, nant, maxR), dtype=torch.float64, device="cuda")
    for e in range(E):
        n = int(b.nrules[e])
        store[e, :, :n] = dev(b.u[np.arange(nant)[:, None], b.uidx[e, :, :n]])
    envs = frirl_amd.Envs(prob, "cuda", rant_init=store)
    envs.spread_ant.copy_(dev(spread))
    envs.spread_R.copy_(dev(b.nrules))
    weights = torch.zeros((E, maxR), dtype=torch.float64, device="cuda")
    frirl_amd.check(frirl_amd.lib().frirl_hip_weights_from_spread(C.byref(prob.tables), C.byref(prob.bases), p, C.byref(envs.desc),
                                                                  C.c_void_p(weights.data_ptr()), None), "frirl_hip_weights_from_spread")
    torch.cuda.synchronize()
    w = weights.cpu().numpy()
    for e in range(E):
        n = int(b.nrules[e])
        assert rel(w[e, :n], fives[e].weights[:n]).max() <= RTOL, e
        assert (w[e, n:] == 0).all() and int(envs.spread_R[e]) == 0
    R_before = [f.R for f in fives]
    q_before = [np.array(f.rconc[: f.R]).copy() for f in fives]
    full = prob.merge_rb(agent, dev(srant), dev(srconc), weights, rant_store=store)
    torch.cuda.synchronize()
    assert (full.cpu().numpy() == 0).all()
    nr, rb, st = prob.nrules.cpu().numpy(), prob.rb.cpu().numpy(), store.cpu().numpy()
    inserted = changed = 0
    for e in range(E):
        f = fives[e]
        f.merge_rb(oag, srant, srconc)
        R1 = f.R
        assert nr[e] == R1, (e, nr[e], R1)
        assert (st[e, :, :R1].T == np.array(f.rant[:R1])).all(), "antecedents / rule order"
        assert (rb[e, :nant, :R1] == np.array(f.veval[:, :R1])).all()
        ref = np.array(f.rconc[:R1])
        assert (np.abs(rb[e, nant, :R1] - ref) / np.maximum(np.abs(ref), 1e-9)).max() <= 1e-9, e
        inserted += R1 - R_before[e]
        changed += int((ref[: R_before[e]] != q_before[e]).sum())
    assert inserted > 0 and changed > 0, (inserted, changed)
