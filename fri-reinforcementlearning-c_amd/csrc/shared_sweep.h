// shared_sweep.h -- the sweep of ONE shared, read-only rule base by many lanes (split out of shared.hip so that the caller-stepped
// policy kernels, policy_kernel.h, instantiate the same code): LDS tile, one lane's conclusions, first maximum over a lane group.
#pragma once
#include "sweeps.h"
#include <type_traits>

namespace frirl {

constexpr int SH_TILE = 256;   // rules per LDS tile
constexpr int SH_BLOCK = 256;

template <int NANT>
struct SharedTile {
    double col[(NANT + 1) * SH_TILE];
    uint8_t slot[SH_TILE];
    double ave[FRIRL_HIP_MAX_ACTIONS];
};

// One lane's conclusions against the whole shared rule base; every lane of the workgroup must call it (barriers).
//   GBA: q[] holds the nant-1 state VE points, the action VE points come from tl.ave; conclusions of all A actions go
//        to conc[0..A) (if non-NULL) and the first maximum (frirl_get_best_action.c:60-75) is returned in bi.
//   !GBA: q[] holds all nant VE points; conc[0] / hit0 are FIVE_vag_concl's result.
//   EXCL: rules whose candidate slot s (slot_g[r], 255 = none) has bit s set in `mask` are treated as removed
//        (same sums and same first-hit ORDER as the compacted rule base: removal keeps the relative rule order,
//        five_remove_rule.c:29-85).
//   H > 1: H lanes (G apart, slice index h) share every conclusion of this lane: lane h takes the rules r = h (mod H); the
//        partial sums are added in slice order and the lowest exact hit wins (latency form for few environments).
template <int NANT, int AMAX, bool GBA, bool EXCL, int G = 1, int H = 1, class POW = PowU>
__device__ __forceinline__ void shared_sweep(SharedTile<NANT> &tl, const double *__restrict__ rb, const uint8_t *__restrict__ slot_g, int R,
                                             int maxR, POW p, int abeg, int aend, int nchunks, const double *q, bool live, uint32_t mask,
                                             double *conc, unsigned &hit0, int &bi, double &bvout, int h = 0)
{
    constexpr int NS = NANT - 1;
    constexpr int ND = GBA ? NS : NANT;
    const double *qcol = rb + (size_t)NANT * maxR;
    const int nact = GBA ? aend : 1;
    // running first maximum over this lane's actions [abeg, aend): `bv < c` as max.inl:21; action 0 always seeds it (so a
    // NaN there sticks, as in the reference), a lane that starts later seeds with -inf and skips NaNs
    double bv = -__builtin_inf();
    bi = abeg;
    hit0 = FRIRL_HIP_NO_HIT;
    const auto pk = pin_pow(p);            // series coefficients of the Shepard weight in registers (sweeps.h)
    // actions in chunks of AMAX accumulators (A = 21: three passes over the L2-resident rule base keep the kernel at
    // ~90 VGPRs instead of 254)
    // `nchunks` is uniform over the workgroup (the tile staging below has barriers); a lane with fewer actions idles
    for (int c = 0; c < nchunks; c++) {
        const int a0 = (GBA ? abeg : 0) + c * AMAX;
        const int left = nact - a0;
        const int nacc = left < 0 ? 0 : (left < AMAX ? left : AMAX);
        double sv[AMAX], sw[AMAX];
        unsigned sh[AMAX];
#pragma unroll
        for (int a = 0; a < AMAX; a++) { sv[a] = 0.0; sw[a] = 0.0; sh[a] = FRIRL_HIP_NO_HIT; }
        for (int r0 = 0; r0 < R; r0 += SH_TILE) {
            const int n = (R - r0 < SH_TILE) ? R - r0 : SH_TILE;
            __syncthreads();
            for (int i = threadIdx.x; i < (NANT + 1) * SH_TILE; i += SH_BLOCK) {
                const int k = i / SH_TILE, r = i - k * SH_TILE;
                tl.col[i] = (r < n) ? rb[(size_t)k * maxR + r0 + r] : 0.0;
            }
            if (EXCL) for (int r = threadIdx.x; r < SH_TILE; r += SH_BLOCK) tl.slot[r] = (r < n) ? slot_g[r0 + r] : (uint8_t)255;
            __syncthreads();
            if (live && nacc > 0) {
                // branch-free body (selects on the exact-hit test and on the try-remove mask): straight-line code per rule
                for (int r = h; r < n; r += H) {
                    bool valid = true;
                    if (EXCL) { const unsigned sl = tl.slot[r]; valid = !(sl < 32u && ((mask >> sl) & 1u)); }
                    double d0 = q[0] - tl.col[r];
                    double s = d0 * d0;
#pragma unroll
                    for (int k = 1; k < ND; k++) { const double d = q[k] - tl.col[k * SH_TILE + r]; s = __fma_rn(d, d, s); }
                    const double cq = tl.col[NANT * SH_TILE + r];
                    // a removed rule gets a huge squared distance once (its weight vanishes: the sums keep the bits of the compacted
                    // rule base); an exact hit is noted with a select and poisons the sums of its own conclusion, which are then not
                    // read (sweeps.h: q_pair) -- no select around the weight
                    if (EXCL) s = valid ? s : NO_RULE_STATE_PART;
                    if (GBA) {
                        const double va = tl.col[NS * SH_TILE + r];
#pragma unroll
                        for (int a = 0; a < AMAX; a++) {
                            if (a < nacc) {
                                const double e = tl.ave[a0 + a] - va;
                                const double d2 = __fma_rn(e, e, s);
                                const double wi = shepard_w(d2, pk);
                                sv[a] = __fma_rn(wi, cq, sv[a]);
                                sw[a] = sw[a] + wi;
                                sh[a] = (d2 == 0.0 && sh[a] == FRIRL_HIP_NO_HIT) ? (unsigned)(r0 + r) : sh[a];
                            }
                        }
                    } else {
                        const double wi = shepard_w(s, pk);
                        sv[0] = __fma_rn(wi, cq, sv[0]);
                        sw[0] = sw[0] + wi;
                        sh[0] = (s == 0.0 && sh[0] == FRIRL_HIP_NO_HIT) ? (unsigned)(r0 + r) : sh[0];
                    }
                }
            }
        }
        if (H > 1 && live) {             // combine the H rule slices (all lanes of an environment are live together)
            const int lane = threadIdx.x & (FRIRL_WAVE - 1);
            const int first = lane - h * G;
#pragma unroll
            for (int a = 0; a < AMAX; a++) {
                double tv = __shfl(sv[a], first), tw = __shfl(sw[a], first);
                unsigned th = (unsigned)__shfl((int)sh[a], first);
#pragma unroll
                for (int hh = 1; hh < H; hh++) {
                    const double v = __shfl(sv[a], first + hh * G), w = __shfl(sw[a], first + hh * G);
                    const unsigned x = (unsigned)__shfl((int)sh[a], first + hh * G);
                    tv = tv + v;
                    tw = tw + w;
                    th = x < th ? x : th;
                }
                sv[a] = tv; sw[a] = tw; sh[a] = th;
            }
        }
        if (live) {
#pragma unroll
            for (int a = 0; a < AMAX; a++) {
                if (a < nacc) {
                    const double c = (sh[a] != FRIRL_HIP_NO_HIT) ? qcol[sh[a]] : sv[a] / sw[a];
                    if (conc) conc[a0 + a] = c;
                    if (a0 + a == 0 || bv < c) { bv = c; bi = a0 + a; }
                }
            }
            if (c == 0) hit0 = sh[0];
        }
    }
    bvout = bv;
}

// First maximum over the G lanes that share one environment (consecutive lanes of one wave, each holding the first
// maximum of its own block of actions): combined in block order with the reference's `bv < c` (max.inl:21).
template <int G>
__device__ __forceinline__ void group_first_max(double &bv, int &bi)
{
    if (G == 1) return;
    const int lane = threadIdx.x & (FRIRL_WAVE - 1);
    const int base = lane - (lane % G);
    double cb = __shfl(bv, base);
    int ci = __shfl(bi, base);
#pragma unroll
    for (int g = 1; g < G; g++) {
        const double v = __shfl(bv, base + g);
        const int i = __shfl(bi, base + g);
        if (cb < v) { cb = v; ci = i; }
    }
    bv = cb;
    bi = ci;
}

// The share of a row's group of G * H consecutive lanes that one lane takes in shared_sweep: rule slice h and action slot sub, which
// serves the actions [abeg, aend) in nchunks passes of AMAX accumulators (nchunks is uniform over the workgroup).
struct GroupLane {
    int sub, h, abeg, aend, nchunks;
    bool leader;                   // the lane that answers for the row
};

template <int G, int H, int AMAX>
__device__ __forceinline__ GroupLane group_lane(int A)
{
    GroupLane l;
    const int gl = threadIdx.x % (G * H);
    l.sub = gl % G;
    l.h = gl / G;
    l.leader = gl == 0;
    const int apl = (A + G - 1) / G;                                 // actions per lane
    l.abeg = (l.sub * apl < A) ? l.sub * apl : A;
    l.aend = (l.abeg + apl < A) ? l.abeg + apl : A;
    l.nchunks = (apl + AMAX - 1) / AMAX;
    return l;
}

// The agent's grids ([NANT * FRIRL_HIP_MAX_GRID] doubles of LDS) and action VE points for the workgroup; the first barrier of
// shared_sweep comes before anything reads them.
template <int NANT>
__device__ __forceinline__ void stage_agent(SharedTile<NANT> &tl, double *grid_s, const frirl_hip_agent &ag)
{
    for (int i = threadIdx.x; i < NANT * FRIRL_HIP_MAX_GRID; i += SH_BLOCK) grid_s[i] = ag.grid_values[i];
    if ((int)threadIdx.x < ag.A) tl.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
}

// The Shepard power of a kernel of the shape ladder: PN = the power is the antecedent count, known at compile time; else the agent's.
template <int NANT, bool PN>
using KernelPow = typename std::conditional<PN, PowC<NANT>, PowU>::type;

template <int NANT, bool PN>
__device__ __forceinline__ KernelPow<NANT, PN> kernel_pow(const frirl_hip_agent &ag)
{
    KernelPow<NANT, PN> p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;
    return p;
}

// Rows of agent e that a batched roll-out serves: row_count[e] (NULL = n) clamped to 0..n, and none for an inactive agent or one whose
// rule count lies outside 1..maxR.
__device__ __forceinline__ int agent_rows(const int32_t *__restrict__ row_count, const uint8_t *__restrict__ active, int n,
                                          const int32_t *__restrict__ nrules, int maxR, int e)
{
    int rows = row_count ? row_count[e] : n;
    rows = rows < 0 ? 0 : (rows > n ? n : rows);
    const int R = nrules[e];
    if ((active && active[e] == 0) || R < 1 || R > maxR) rows = 0;
    return rows;
}

// Appends the flagged threads of a workgroup of BLOCK threads, in thread order, to a list that holds `count` of at most `cap` entries.
// Returns this thread's position (to be written only if flagged and < cap) and updates count / over, the same in every thread.
// Every thread must call it (one barrier inside); wave_cnt: one int of LDS per wave.  The caller writes its entry and then
// passes a barrier of its own before the next call: wave_cnt is rewritten there, and the entries written become visible.
template <int BLOCK>
__device__ __forceinline__ int block_append(bool flag, int (&wave_cnt)[BLOCK / FRIRL_WAVE], int cap, int &count, int &over)
{
    const int lane = threadIdx.x & (FRIRL_WAVE - 1), wave = threadIdx.x / FRIRL_WAVE;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = count + __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
    for (int i = 0; i < BLOCK / FRIRL_WAVE; i++) { pos += i < wave ? wave_cnt[i] : 0; tot += wave_cnt[i]; }
    over |= count + tot > cap ? 1 : 0;
    count = count + tot > cap ? cap : count + tot;
    return pos;
}

}  // namespace frirl
