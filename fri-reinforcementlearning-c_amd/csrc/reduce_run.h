// reduce_run.h -- ReduceRun: the host state of ONE batched reduction and every launch of its protocol kernels (reduce_run.hip).
// A run is: init (argument checks, no device) -> start (order kernel) -> per round { the replays; close } -> results.  What a run
// does NOT own is who runs the replays of a round: frirl_hip_reduce_batch and frirl_hip_reduce_batch_starts launch their roll-out
// kernel over rows_per_agent() rows of the nlive() agents of list cur(); frirl_hip_batch_reducer_* lets the caller step them.
#pragma once
#include "reduce_ws.h"

struct ReduceRun {
    frirl_hip_tables t;
    frirl_hip_rulebases b;
    frirl_hip_agent agent;                    // greedy copy (no_random = 1: reduction_state == 1 keeps epsilon at 0 in every demo)
    double *rant = nullptr;
    double reward_good_above = 0.0, reward_tolerance = 0.0;
    int strategy = 0, depth = 0, nodes = 0;
    int ns = 0, drop_bad = 0;                 // start states per agent (0: none, one row per node) and drop_bad_starts
    bool stepped = false;                     // the caller steps the replays: a node's starts sit at node * ns + k, not node * K_e + ki
    size_t need = 0;                          // bytes of the workspace (what the matching *_workspace_bytes function answers)
    hipStream_t s = nullptr;
    ReduceBatchWs ws;                         // == sw.b where there are start states
    ReduceStartsWs sw = {};
    int32_t hdr[4] = {0, 0, 0, 0};            // host copy of ws.hdr: live agents of even / odd rounds, bad agent + 1, rows live
    int round = 0;                            // round 0 = the baseline replays

    // Checks strategy, depth, the number of start states (`starts` NULL: none), A / max_steps and the rows of a round, resolves depth
    // 0 by the depth rule and fills the state.  Looks at no device; 0 or FRIRL_HIP_EINVAL with the reason after "who: ".
    int init(const char *who, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
             const frirl_hip_reduce_starts *starts, int strategy, double reward_tolerance, int depth, bool stepped, void *stream);
    int check_workspace(const char *who, const void *workspace, size_t bytes) const;      // a caller's workspace: pointer, alignment, `need`
    // carves `workspace`, zeroes the header, runs the order (and init) kernel and reads the header: refuses a bad nrules.  Synchronises.
    int start(const char *who, void *workspace, const uint8_t *active, const int32_t *start_count);

    int cur() const { return round & 1; }                             // index of this round's live list
    int nlive() const { return hdr[round & 1]; }                      // agents of this round; 0: the run has ended
    bool first() const { return round == 0; }
    int per_node() const { return ns ? ns : 1; }
    int rows_per_agent() const { return (round == 0 ? 1 : nodes) * per_node(); }

    int header(const char *who);              // the 16-byte header to the host; synchronises
    // the close kernel of this round, the header (the next round's live count), round + 1, and the next round's open kernel
    int close(const char *who);
    // result kernels and downloads: results [E] (+ kept [E][maxR], may be NULL), per_start [E][ns]; either may be NULL.  Synchronises.
    int results(const char *who, int32_t *kept, frirl_hip_reduce_result *results, frirl_hip_reduce_start_result *per_start);
};
