// reduce_map_ws.h -- the arrays of one map-validated reduction (frirl_hip_reduce_batch_map), carved out of one workspace, and the
// launches of its kernels.  The kernels (reduce_map_kernels.h) sit in reduce_run.hip's translation unit, beside the order kernel and the
// compaction they reuse (reduce_batch_kernels.h): the library is built without relocatable device code.  No kernel is defined here.
#pragma once
#include "reduce_ws.h"
#include "policy_map_sweep.h"

namespace frirl {

struct ReduceMapWs {
    ReduceBatchWs b;              // of depth 1: hdr, order, alive, slot (255 = present, 0 = removed) and R0 are used
    double *qve;                  // [E][n][nant-1] the VE points of the agents' points
    int32_t *best0;               // [E][n] the map of the un-reduced rule bases
    frirl_hip_reduce_map_result *res;      // [E]
};

// what a map or a map-validated reduction reads besides the rule bases
struct MapArgs {
    const double *u, *ve;         // the tables
    int U, A, p, n;
    const double *action_ve, *points;
    const int32_t *point_count;
    const uint8_t *active;
};

}  // namespace frirl

using frirl::ReduceMapWs;

static size_t reduce_map_layout(char *base, size_t E, size_t maxR, size_t n, int nant, ReduceMapWs *ws)
{
    ReduceMapWs w;
    size_t off = reduce_batch_layout(base, E, maxR, 1, E, &w.b);
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    w.qve = reinterpret_cast<double *>(take(sizeof(double) * E * n * (size_t)(nant - 1)));
    w.best0 = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * n));
    w.res = reinterpret_cast<frirl_hip_reduce_map_result *>(take(sizeof(frirl_hip_reduce_map_result) * E));
    if (ws) *ws = w;
    return off;
}

// reduce_run.hip.  Order: zeroes the header and ranks every agent's |Q| (reduce_batch_order_kernel); the header then holds the first
// active agent with nrules outside 1..maxR (+ 1) in hdr[2].  Run: the whole try-remove of every agent, one launch, then the results.
int reduce_map_launch_order(const char *who, const frirl_hip_tables &t, const frirl_hip_rulebases &b, const uint8_t *active, int strategy,
                            const ReduceMapWs &ws, hipStream_t s);      // 0 or FRIRL_HIP_ELAUNCH
void reduce_map_launch_run(const frirl_hip_tables &t, const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident,
                           const ReduceMapWs &ws, hipStream_t s);

// ---- argument checks shared by policy_map.hip and rule_usage.hip (no device is looked at; the workspace: check_workspace, batch_shape.h) ----
// the checks the map and the map-validated reduction share; fills `m`
static int check_map_args(const char *who, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                          const frirl_hip_map_points *pts, frirl::MapArgs *m)
{
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!agent || !agent->action_ve || !pts || !pts->points) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (t->nant < 2 || t->nant > 8) { set_error("%s: nant=%d outside 2..8", who, t->nant); return FRIRL_HIP_EINVAL; }
    if (agent->A < 1 || agent->A > FRIRL_HIP_MAX_ACTIONS) { set_error("%s: A=%d outside 1..%d", who, agent->A, FRIRL_HIP_MAX_ACTIONS); return FRIRL_HIP_EINVAL; }
    if (pts->n < 1 || (long long)b->E * pts->n > INT32_MAX) { set_error("%s: n=%d points per agent (E=%d): n < 1 or E * n > 2^31 - 1", who, pts->n, b->E); return FRIRL_HIP_EINVAL; }
    m->u = t->u; m->ve = t->ve; m->U = t->U;
    m->A = agent->A; m->p = agent->p > 0 ? agent->p : t->nant; m->n = pts->n;
    m->action_ve = agent->action_ve; m->points = pts->points; m->point_count = pts->point_count; m->active = pts->active;
    return FRIRL_HIP_OK;
}
