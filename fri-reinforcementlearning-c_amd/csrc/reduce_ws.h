// reduce_ws.h -- the arrays of one batched reduction, carved out of one workspace: ReduceBatchWs (per agent and per tree node),
// ReduceStartsWs (the same plus the per-start arrays of a run against a set of start states) and their layout functions.  No kernel
// is defined here: the roll-out kernels (reduce_batch.hip, reduce_starts.hip), the caller-stepped reducer (policy_batch.hip) and the
// driver of the protocol kernels (ReduceRun, reduce_run.h) all see the arrays through these structs.
#pragma once
#include "reduce_walk.h"
#include "batch_shape.h"

namespace frirl {

// the arrays of one call, carved out of the caller's workspace (reduce_batch_layout)
struct ReduceBatchWs {
    int32_t *hdr;                 // [4] live count of even rounds, of odd rounds, first agent with a bad rule count + 1, rows still live
    uint32_t *mask;               // [nodes] exclude mask of every tree node: the same for every agent
    int32_t *live[2];             // [E] agents still reducing, this round's list and the next one's
    int32_t *order;               // [E][maxR] candidates in trial order (original rule indices)
    int32_t *alive;               // [E][maxR] original index of the rule in each current slot
    uint8_t *slot;                // [E][maxR] candidate slot of every current rule in this round, 255 = none
    int32_t *steps;               // [E][nodes] replay results of this round
    double *reward;               // [E][nodes]
    int32_t *j, *d, *R0, *rounds, *rollouts, *steps_inc, *cap;      // [E]
    double *prev;                 // [E] prev_reward
    frirl_hip_reduce_result *res; // [E]
    int nodes;                    // 2^depth - 1
};

// the arrays of one call: those of the batched reduction (b.steps / b.reward hold nodes * n entries per agent) and the per-start ones
struct ReduceStartsWs {
    ReduceBatchWs b;
    int32_t *cnt;                 // [E] participating starts: start_count[e] clamped to 1..n
    int32_t *K;                   // [E] used starts (after the baseline)
    int32_t *capmax;              // [E] largest cap of a used start: the roll-out kernel's loop bound
    int32_t *used;                // [E][n] the used starts in ascending order (first K[e] entries)
    int32_t *steps_inc;           // [E][n] per start: steps of the baseline replay, -1 = takes no part
    int32_t *cap;                 // [E][n] per start: min(max_steps, steps_inc + 1)
    double *prev;                 // [E][n] per start: prev_reward
    frirl_hip_reduce_start_result *res;      // [E][n]
    int n;                        // starts per agent
};

}  // namespace frirl

using namespace frirl_host;
using frirl::ReduceBatchWs;
using frirl::ReduceStartsWs;

// rb_group, rb_resident_rows, rb_slices, up16: batch_shape.h (shared with the batched roll-outs, rollout_batch.hip)

// carves the arrays of a call out of `base` (NULL: sizes only); `rows` = entries of steps / reward
static size_t reduce_batch_layout(char *base, size_t E, size_t maxR, int depth, size_t rows, ReduceBatchWs *ws)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    ReduceBatchWs w;
    w.nodes = frirl::rw_nodes(depth);
    w.hdr = reinterpret_cast<int32_t *>(take(4 * sizeof(int32_t)));
    w.mask = reinterpret_cast<uint32_t *>(take(sizeof(uint32_t) * w.nodes));
    w.live[0] = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.live[1] = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.order = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * maxR));
    w.alive = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * maxR));
    w.slot = reinterpret_cast<uint8_t *>(take(E * maxR));
    w.steps = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * rows));
    w.reward = reinterpret_cast<double *>(take(sizeof(double) * rows));
    int32_t **per_agent[] = {&w.j, &w.d, &w.R0, &w.rounds, &w.rollouts, &w.steps_inc, &w.cap};
    for (int32_t **p : per_agent) *p = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.prev = reinterpret_cast<double *>(take(sizeof(double) * E));
    w.res = reinterpret_cast<frirl_hip_reduce_result *>(take(sizeof(frirl_hip_reduce_result) * E));
    if (ws) *ws = w;
    return off;
}

static size_t reduce_starts_layout(char *base, size_t E, size_t maxR, int depth, size_t rows, int n, ReduceStartsWs *ws)
{
    ReduceStartsWs w;
    size_t off = reduce_batch_layout(base, E, maxR, depth, rows, &w.b);
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    w.n = n;
    int32_t **per_agent[] = {&w.cnt, &w.K, &w.capmax};
    for (int32_t **p : per_agent) *p = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    int32_t **per_start[] = {&w.used, &w.steps_inc, &w.cap};
    for (int32_t **p : per_start) *p = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * n));
    w.prev = reinterpret_cast<double *>(take(sizeof(double) * E * n));
    w.res = reinterpret_cast<frirl_hip_reduce_start_result *>(take(sizeof(frirl_hip_reduce_start_result) * E * n));
    if (ws) *ws = w;
    return off;
}
