// reduce_walk.h -- the order and walk logic of the speculative try-remove reduction (frirl_sequential_run.c:170-350) as
// __host__ __device__ inline functions: candidate rank, tree node <-> exclude mask, the walk along the outcomes that happened and
// the keep flags.  The kernels of the batched reduction (reduce_batch.hip) call them on the device; the host-only probe
// frirl_hip_reduce_walk_check runs the same walk on host arrays, so the CPU suite can pin it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace frirl {

constexpr int RW_MAX_DEPTH = 12;                 // candidates per round; a round's tree has 2^d - 1 nodes

// Is rule q tried before rule r?  Stable order by |Q|: ascending for strategy 1 (the reference rescans for the FIRST minimum,
// `mvalue > fabs(..)` :268), descending for strategy 2 (the first maximum, :286).  aq / ar = |Q_q| / |Q_r|, finite.
// rank[r] = #{q : rw_before(q, r)} = #{q : |Q_q| < |Q_r|} + #{q < r : |Q_q| == |Q_r|}   (mirrored for strategy 2)
__host__ __device__ inline bool rw_before(double aq, int q, double ar, int r, int strategy)
{
    return (strategy == 1 ? aq < ar : aq > ar) || (aq == ar && q < r);
}

__host__ __device__ inline int rw_nodes(int d) { return (1 << d) - 1; }

// node (k, bits): candidates j .. j+k-1 had the outcomes `bits` (1 = removed), candidate j+k is on trial
__host__ __device__ inline uint32_t rw_node(int k, uint32_t bits) { return (1u << k) - 1u + bits; }

// exclude mask of a node: the removals on the way to it and the candidate on trial
__host__ __device__ inline uint32_t rw_node_mask(uint32_t node)
{
    int k = 0;
    while ((2u << k) <= node + 1u) k++;
    const uint32_t bits = node + 1u - (1u << k);
    return bits | (1u << k);
}

// the acceptance test of frirl_sequential_run.c:212
__host__ __device__ inline bool rw_accept(int steps, double reward, int steps_inc, double prev_reward, double good_above, double tol)
{
    const double diff = prev_reward - reward;
    return reward > good_above && steps == steps_inc && fabs(diff) <= tol;
}

// Walk a round's tree along the outcomes that happened (steps / reward: one entry per node); returns the removal bits of its d
// candidates and carries prev_reward from accepted removal to accepted removal (:222).
__host__ __device__ inline uint32_t rw_walk(int d, const int32_t *steps, const double *reward, int steps_inc, double &prev_reward, double good_above,
                                            double tol)
{
    uint32_t bits = 0;
    for (int k = 0; k < d; k++) {
        const uint32_t node = rw_node(k, bits);
        if (rw_accept(steps[node], reward[node], steps_inc, prev_reward, good_above, tol)) {
            bits |= 1u << k;
            prev_reward = reward[node];
        }
    }
    return bits;
}

// The same walk with K replays per node, the node's replay from the ki-th used start state: a removal is accepted iff rw_accept holds
// for EVERY start, and then every start's prev_reward moves to its own replay's reward (:222, per start).  steps_inc / prev_reward
// are indexed by the start's number used[ki] (used == NULL: by ki itself).  A node's replays sit `stride` entries apart from the next
// node's, the ki-th at column ki (by_start == false; the compact form is stride == K) or at column used[ki] (by_start: the
// caller-stepped form, one column per start whether used or not, stride == n).  K == 1 is rw_walk.
// All K tests of a node are evaluated (no early exit): their loads do not depend on each other.
__host__ __device__ inline uint32_t rw_walk_starts(int d, int K, int stride, bool by_start, const int32_t *steps, const double *reward,
                                                   const int32_t *used, const int32_t *steps_inc, double *prev_reward, double good_above, double tol)
{
    uint32_t bits = 0;
    for (int k = 0; k < d; k++) {
        const size_t row = (size_t)rw_node(k, bits) * stride;
        bool all = true;
        for (int ki = 0; ki < K; ki++) {
            const int s = used ? used[ki] : ki, c = by_start ? s : ki;
            all = rw_accept(steps[row + c], reward[row + c], steps_inc[s], prev_reward[s], good_above, tol) && all;
        }
        if (!all) continue;
        bits |= 1u << k;
        for (int ki = 0; ki < K; ki++) {
            const int s = used ? used[ki] : ki;
            prev_reward[s] = reward[row + (by_start ? s : ki)];
        }
    }
    return bits;
}

// keep flag of a rule with candidate slot `slot` (255 = not a candidate of this round) after a walk that ended with `bits`
__host__ __device__ inline bool rw_dropped(unsigned slot, uint32_t bits) { return slot < 32u && ((bits >> slot) & 1u); }

}  // namespace frirl
