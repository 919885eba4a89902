// policy_map_sweep.h -- the greedy action of ONE rule base at many points ("policy map"; include/frirl_hip.h: frirl_hip_policy_map,
// frirl_hip_reduce_batch_map): device functions shared by the map kernel (policy_map.hip) and the try-remove kernel
// (reduce_map_kernels.h).  No kernel is defined here.
//
// Lane = (point, block of AMAX actions).  A lane walks ALL rules in ascending index order and keeps its own Shepard sums, so every
// conclusion is accumulated by one lane in the order of five_hip_vag_concl_shared (shared_sweep.h) and its bits depend on the rule
// base, the point and the action alone -- not on n, E, AMAX, the launch shape or where the rules are read from (LDS or global).
// A rule that is absent (`gone[r] != 255`, the slot-table encoding of reduce_ws.h) or on trial (`r == cand`) is SKIPPED, not
// down-weighted: the additions that remain are those of the compacted rule base in the same order, hence bit-identical to its map.
#pragma once
#include "sweeps.h"

namespace frirl {

constexpr int PM_BLOCK = 256;

// lanes of a 256-thread workgroup over points: `chunks` consecutive lanes share a point, each with its own block of AMAX actions
struct MapShape {
    int chunks;      // ceil(A / AMAX)
    int ppp;         // points per pass of the workgroup: PM_BLOCK / chunks
};
__host__ __device__ inline MapShape map_shape(int A, int amax)
{
    MapShape s;
    s.chunks = (A + amax - 1) / amax;
    s.ppp = PM_BLOCK / s.chunks;
    return s;
}

// The conclusions of actions [a0, a0 + nacc) at the VE point q, and their first maximum (bv, bi) in the reference's form (`bv < c`,
// max.inl:21): action 0 always seeds it, a lane that starts later seeds with -inf and so skips NaNs -- shared_sweep's rule.
//   cols   the rule base's columns, column k at cols + k * stride (LDS or global; the compiler follows the address space after inlining)
//   gone   per-rule slot byte, 255 = present, anything else = removed earlier in this run (NULL: all present);  cand: the rule on trial, -1 = none
//   ave    the action VE points (LDS)
template <int NANT, int AMAX>
__device__ __forceinline__ void map_conclusions(const double *cols, size_t stride, const uint8_t *gone, int R, int cand, PowU p, const double *ave,
                                                int a0, int nacc, const double (&q)[NANT - 1], double *conc, double &bv, int &bi)
{
    constexpr int NS = NANT - 1;
    double sv[AMAX], sw[AMAX];
    unsigned sh[AMAX];
    double av[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; a++) { sv[a] = 0.0; sw[a] = 0.0; sh[a] = FRIRL_HIP_NO_HIT; av[a] = a < nacc ? ave[a0 + a] : 0.0; }
    for (int r = 0; r < R; r++) {
        if (r == cand || (gone && gone[r] != 255)) continue;                  // uniform over the workgroup
        const double d0 = q[0] - cols[r];
        double s = d0 * d0;
#pragma unroll
        for (int k = 1; k < NS; k++) { const double d = q[k] - cols[k * stride + r]; s = __fma_rn(d, d, s); }
        const double va = cols[NS * stride + r], cq = cols[NANT * stride + r];
#pragma unroll
        for (int a = 0; a < AMAX; a++) {
            if (a < nacc) {
                const double e = av[a] - va;
                const double d2 = __fma_rn(e, e, s);
                // an exact hit poisons the sums of its own conclusion (1 / 0), which are then not read
                const double wi = shepard_w(d2, p);
                sv[a] = __fma_rn(wi, cq, sv[a]);
                sw[a] = sw[a] + wi;
                sh[a] = (d2 == 0.0 && sh[a] == FRIRL_HIP_NO_HIT) ? (unsigned)r : sh[a];
            }
        }
    }
    bv = -__builtin_inf();
    bi = a0;
#pragma unroll
    for (int a = 0; a < AMAX; a++) {
        if (a < nacc) {
            const double c = (sh[a] != FRIRL_HIP_NO_HIT) ? cols[NANT * stride + sh[a]] : sv[a] / sw[a];
            if (conc) conc[a0 + a] = c;
            if (a0 + a == 0 || bv < c) { bv = c; bi = a0 + a; }
        }
    }
}

// The squared VE distance of rule r to (q, av) in map_conclusions' operations and FMA chain: the same bits as its d2.
template <int NANT>
__device__ __forceinline__ double map_rule_d2(const double *cols, size_t stride, int r, const double (&q)[NANT - 1], double av)
{
    const double d0 = q[0] - cols[r];
    double s = d0 * d0;
#pragma unroll
    for (int k = 1; k < NANT - 1; k++) { const double d = q[k] - cols[k * stride + r]; s = __fma_rn(d, d, s); }
    const double e = av - cols[(NANT - 1) * stride + r];
    return __fma_rn(e, e, s);
}

// One more walk for a SINGLE action (rule usage, rule_usage.hip): the Shepard weight sum of the action VE point `av` at q over all R
// rules in ascending order -- the bits of map_conclusions' sw for that action -- and the first exact hit (FRIRL_HIP_NO_HIT = none).
template <int NANT>
__device__ __forceinline__ void map_weight_sum(const double *cols, size_t stride, int R, PowU p, const double (&q)[NANT - 1], double av, double &S,
                                               unsigned &hit)
{
    S = 0.0;
    hit = FRIRL_HIP_NO_HIT;
    for (int r = 0; r < R; r++) {
        const double d2 = map_rule_d2<NANT>(cols, stride, r, q, av);
        S = S + shepard_w(d2, p);
        hit = (d2 == 0.0 && hit == FRIRL_HIP_NO_HIT) ? (unsigned)r : hit;
    }
}

// LDS of one pass: the first maximum of every lane, combined per point in block order
struct MapPassLds {
    double bv[PM_BLOCK];
    int bi[PM_BLOCK];
};

// One pass of the workgroup over the points [pt0, pt0 + shape.ppp) of one agent: every lane its block of actions, then the lane of
// block 0 combines its point's blocks in block order (group_first_max's rule).  Returns the point's greedy action in the lane of
// block 0 of an existing point, -1 in every other lane.  Every thread of the workgroup calls it (two barriers).
//   qve    [cnt][NANT-1] the VE points of the agent's points;  conc: [cnt][A] or NULL
template <int NANT, int AMAX>
__device__ __forceinline__ int map_pass(MapPassLds &pl, const double *cols, size_t stride, const uint8_t *gone, int R, int cand, PowU p, const double *ave,
                                        int A, MapShape shape, const double *qve, int pt0, int cnt, double *conc)
{
    constexpr int NS = NANT - 1;
    const int tid = threadIdx.x;
    const int pl_pt = tid / shape.chunks, chunk = tid - pl_pt * shape.chunks;
    const int pt = pt0 + pl_pt;
    const bool live = pl_pt < shape.ppp && pt < cnt;
    const int a0 = chunk * AMAX;
    const int left = A - a0;
    const int nacc = left < AMAX ? left : AMAX;
    double bv = -__builtin_inf();
    int bi = a0;
    if (live) {
        double q[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) q[k] = qve[(size_t)pt * NS + k];
        map_conclusions<NANT, AMAX>(cols, stride, gone, R, cand, p, ave, a0, nacc, q, conc ? conc + (size_t)pt * A : nullptr, bv, bi);
    }
    pl.bv[tid] = bv;
    pl.bi[tid] = bi;
    __syncthreads();
    int best = -1;
    if (live && chunk == 0) {
        double cb = bv;
        best = bi;
        for (int g = 1; g < shape.chunks; g++) {
            const double v = pl.bv[tid + g];
            if (cb < v) { cb = v; best = pl.bi[tid + g]; }
        }
    }
    __syncthreads();                                                   // pl is rewritten by the next pass
    return best;
}

// stages the columns of rules [0, R) (global, stride maxR) in LDS with stride `ls`; every thread of the workgroup calls it
template <int NANT>
__device__ __forceinline__ void map_stage(double *lcols, int ls, const double *__restrict__ rb, size_t maxR, int R)
{
    for (int k = 0; k <= NANT; k++)
        for (int r = threadIdx.x; r < R; r += PM_BLOCK) lcols[k * ls + r] = rb[k * maxR + r];
}

// bytes of dynamic LDS per resident rule: its NANT + 1 columns and its flag
__host__ __device__ inline size_t map_rule_bytes(int nant) { return (size_t)(nant + 1) * sizeof(double) + 1; }
constexpr size_t PM_LDS_BUDGET = 56 * 1024;                            // dynamic LDS of the resident forms (64 KiB less the static arrays)
// rules an agent may have to take the resident form: a multiple of 8, so the flag array behind the columns stays 8-byte aligned
__host__ __device__ inline int map_resident_rules(int nant, int maxR)
{
    const size_t cap = (PM_LDS_BUDGET / map_rule_bytes(nant)) & ~(size_t)7, all = ((size_t)maxR + 7) & ~(size_t)7;
    return (int)(cap < all ? cap : all);
}

}  // namespace frirl
