// reduce_orders_ws.h -- the arrays of one map-validated reduction over several candidate orders (frirl_hip_reduce_batch_map_orders;
// DESIGN.md 4b-6), carved out of one workspace, and the launches of its kernels.  The kernels (reduce_orders_kernels.h) sit in
// reduce_run.hip's translation unit, beside the compaction they reuse: the library is built without relocatable device code.  No kernel
// is defined here.
#pragma once
#include "reduce_map_ws.h"

namespace frirl {

struct ReduceOrdersWs {
    int32_t *hdr;                 // [4] first active agent with nrules outside 1..maxR + 1; first (e * K + k) + 1 that is no permutation; unused x 2
    uint8_t *slot;                // [E][K][maxR] PRIVATE slot bytes of every (agent, order): 255 = present, 0 = removed by that order
    int32_t *alive;               // [E][maxR] original index of the rule in each slot (identity until the chosen order is applied)
    double *qve;                  // [E][n][nant-1] the VE points of the agents' points
    int32_t *best0;               // [E][K][n] the map of the un-reduced rule base, one copy per workgroup of the trial launch
    int32_t *after;               // [E][K] rules order k alone leaves
    int32_t *tries;               // [E][K] candidates order k tried
    frirl_hip_reduce_orders_result *res;   // [E]
    int K;
};

}  // namespace frirl

using frirl::ReduceOrdersWs;

static size_t reduce_orders_layout(char *base, size_t E, size_t maxR, size_t n, int nant, size_t K, ReduceOrdersWs *ws)
{
    ReduceOrdersWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    w.K = (int)K;
    w.hdr = reinterpret_cast<int32_t *>(take(4 * sizeof(int32_t)));
    w.slot = reinterpret_cast<uint8_t *>(take(E * K * maxR));
    w.alive = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * maxR));
    w.qve = reinterpret_cast<double *>(take(sizeof(double) * E * n * (size_t)(nant - 1)));
    w.best0 = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * K * n));
    w.after = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * K));
    w.tries = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * K));
    w.res = reinterpret_cast<frirl_hip_reduce_orders_result *>(take(sizeof(frirl_hip_reduce_orders_result) * E));
    if (ws) *ws = w;
    return off;
}

// reduce_run.hip.  Check: zeroes the header, validates the rule counts and every order on the device, snaps the points and fills the
// private slot bytes -- no rule base is written.  Run: the trial launch (one workgroup per agent and order, private slot bytes only) and
// the apply launch (one workgroup per agent: the best order's removals compacted into the rule base), then the results.
int reduce_orders_launch_check(const char *who, const frirl_hip_rulebases &b, const frirl::MapArgs &m, int nant, const int32_t *orders,
                               const ReduceOrdersWs &ws, hipStream_t s);   // 0 or FRIRL_HIP_ELAUNCH
void reduce_orders_launch_run(const frirl_hip_tables &t, const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident,
                              const int32_t *orders, const ReduceOrdersWs &ws, hipStream_t s);
