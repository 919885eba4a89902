// rollout_resident.h -- the LDS-resident rule base of the roll-out kernels: image layout and staging, exact hits by hash lookup and
// the per-lane sweep.  Moved out of rollout.hip (frirl_hip_rollout_shared: ONE rule base per call) so that rollout_batch.hip
// (frirl_hip_rollout_batch: one rule base per AGENT, staged by that agent's workgroups) runs the same code; nothing of it changed on
// the way, and the kernels of rollout.hip compile to the instructions they had before.  resident_sweep is the sweep of
// rollout_resident_kernel as a function; that kernel keeps its inline copy, because calling the function reorders its scalar code.
#pragma once
#include "sweeps.h"

namespace frirl {

// ---- exact hits by lookup ----------------------------------------------------------------------------------------------
// The rule base of a roll-out never changes, so "the lowest rule whose antecedents equal the observation's VE point" (an exact hit:
// distance 0 <=> every antecedent equal, FIVEVagConcl_FRIRL_BestAct.c:89-93) is found through a hash table over the rules' VE
// tuples, built once per workgroup: one probe per action and step instead of a compare + select per action and RULE in the sweep.
constexpr uint32_t HT_EMPTY = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t hash_mix(uint32_t hsh, double x)
{
    const double c = x + 0.0;                             // -0.0 and +0.0 are the same antecedent
    const uint32_t lo = (uint32_t)__double2loint(c), hi = (uint32_t)__double2hiint(c);
    hsh = (hsh ^ lo) * 0x9E3779B1u;
    hsh = (hsh ^ hi) * 0x85EBCA6Bu;
    return hsh ^ (hsh >> 15);
}

// The LDS image of the rule base is rule-major: rule r occupies the NANT + 1 consecutive doubles col[r * (NANT + 1) + k] (antecedent VE
// values, then the consequent) -- one address per rule and 16-byte reads with immediate offsets in the sweep.
template <int NANT>
__device__ __forceinline__ bool rule_equals(const double *col, int, int r, const double (&key)[NANT])
{
    bool eq = true;
#pragma unroll
    for (int k = 0; k < NANT; k++) eq = eq && (col[r * (NANT + 1) + k] == key[k]);
    return eq;
}

template <int NANT>
__device__ __forceinline__ void hash_insert(uint32_t *tab, int ht, const double *col, int RPS, int r)
{
    double key[NANT];
    uint32_t hsh = 0u;
#pragma unroll
    for (int k = 0; k < NANT; k++) { key[k] = col[r * (NANT + 1) + k]; hsh = hash_mix(hsh, key[k]); }
    for (int i = 0; i < ht; i++) {
        const uint32_t slot = (hsh + (uint32_t)i) & (uint32_t)(ht - 1);
        const uint32_t cur = atomicCAS(&tab[slot], HT_EMPTY, (uint32_t)r);
        if (cur == HT_EMPTY) return;
        if (rule_equals<NANT>(col, RPS, (int)cur, key)) { atomicMin(&tab[slot], (uint32_t)r); return; }   // duplicates: the lowest index
    }
}

// lowest rule with these antecedents, or FRIRL_HIP_NO_HIT; `hsh` = hash of key[0 .. NANT-2], the last antecedent is mixed in here
template <int NANT>
__device__ __forceinline__ unsigned hash_lookup(const uint32_t *tab, int ht, const double *col, int RPS, uint32_t hsh, const double (&key)[NANT])
{
    hsh = hash_mix(hsh, key[NANT - 1]);
    for (int i = 0; i < ht; i++) {
        const uint32_t cur = tab[(hsh + (uint32_t)i) & (uint32_t)(ht - 1)];
        if (cur == HT_EMPTY) return FRIRL_HIP_NO_HIT;
        if (rule_equals<NANT>(col, RPS, (int)cur, key)) return cur;
    }
    return FRIRL_HIP_NO_HIT;
}

template <int N>
__device__ __forceinline__ void group_sum_n(double (&v)[N], int H)
{
    for (int off = 1; off < H; off <<= 1) {
        double t[N];
#pragma unroll
        for (int i = 0; i < N; i++) t[i] = __shfl_xor(v[i], off, FRIRL_WAVE);
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = v[i] + t[i];
    }
}

// The canonical columns rb[k][r] of ONE rule base ([NANT+1][maxR], R rules) transposed into the rule-major image col[RPS][NANT+1] by
// `nthr` threads (coalesced reads); the rules R .. RPS-1 are padding: first antecedent 1e150 away (squared distance ~1e300, its
// weight underflows to 0), consequent 0.
template <int NANT>
__device__ __forceinline__ void resident_stage_image(double *col, int RPS, const double *__restrict__ rb, int maxR, int R, int tid, int nthr)
{
    for (int i = tid; i < (NANT + 1) * RPS; i += nthr) {
        const int k = i / RPS, r = i - k * RPS;
        col[r * (NANT + 1) + k] = (r < R) ? rb[(size_t)k * maxR + r] : (k == 0 ? 1.0e150 : 0.0);
    }
}

// This lane's share of frirl_get_best_action's sweep: the rules r = jj * H + h, jj = 0 .. nj-1, of the image for ALL NA actions; the
// state part of the squared distance once per rule.  sv / sw: the lane's partial Shepard sums (the caller adds the H slices).
// Two rules in flight.  A rule's LDS reads are issued right after the first instructions of the PREVIOUS rule's arithmetic -- the ones
// that consume every value that rule read -- so that the compiler's wait for "everything outstanding" (it does not emit partial
// LDS waits across this loop's back edge) falls where only reads issued a whole rule ago are outstanding.  The scheduling
// barriers pin that order; without them the two rules' arithmetic is interleaved and both reads are waited for at once
// (65 536 acrobot roll-outs 9.1 -> 8.3 ms).
// EXCL: slot_s[r] = candidate slot of rule r, a rule whose slot bit is set in `mask` weighs exactly 0 (same sums as the compacted rule base).
template <int NANT, int NA, int H, bool EXCL, class PK>
__device__ __forceinline__ void resident_sweep(const double *col, const uint8_t *slot_s, uint32_t mask, const double (&q)[NANT - 1],
                                               const double (&ave)[NA], const PK &pk, int h, int nj, double (&sv)[NA], double (&sw)[NA])
{
    constexpr int NS = NANT - 1;
    struct Open { double d[NS], va, cq; };
    auto fetch = [&](double (&x)[NANT + 1], int jj) {
        const double *rule = col + (jj * H + h) * (NANT + 1);
#pragma unroll
        for (int k = 0; k <= NANT; k++) x[k] = rule[k];
    };
    auto open = [&](const double (&rule)[NANT + 1]) {              // touches every value of the row
        Open o;
#pragma unroll
        for (int k = 0; k < NS; k++) o.d[k] = q[k] - rule[k];
        o.va = rule[NS]; o.cq = rule[NANT];
        return o;
    };
    auto close = [&](const Open &o, int jj) {
        double s = o.d[0] * o.d[0];
#pragma unroll
        for (int k = 1; k < NS; k++) s = __fma_rn(o.d[k], o.d[k], s);
        if (EXCL) {                               // a removed rule weighs exactly 0 (same sums as the compacted rule base)
            const unsigned sl = slot_s[jj * H + h];
            s = (sl < 32u && ((mask >> sl) & 1u)) ? NO_RULE_STATE_PART : s;
        }
#pragma unroll
        for (int a = 0; a < NA; a++) {
            const double e = ave[a] - o.va;
            const double d2 = __fma_rn(e, e, s);
            const double wi = shepard_w(d2, pk);
            sv[a] = __fma_rn(wi, o.cq, sv[a]);
            sw[a] = sw[a] + wi;
        }
    };
    if (nj > 0) {
        double ra[NANT + 1], rb2[NANT + 1];
        fetch(ra, 0);
        int j = 0;
        for (; j + 1 < nj; j += 2) {
            const Open oa = open(ra);
            __builtin_amdgcn_sched_barrier(0);
            fetch(rb2, j + 1);
            __builtin_amdgcn_sched_barrier(0);
            close(oa, j);
            __builtin_amdgcn_sched_barrier(0);
            const Open ob = open(rb2);
            __builtin_amdgcn_sched_barrier(0);
            fetch(ra, j + 2 < nj ? j + 2 : nj - 1);
            __builtin_amdgcn_sched_barrier(0);
            close(ob, j + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (j < nj) { const Open oa = open(ra); close(oa, j); }
    }
}

}  // namespace frirl
