// reduce_batch.hip -- the rule-base reduction (frirl_sequential_run.c:170-350) of EVERY rule base of a batch in one run of
// speculative try-remove rounds (frirl_hip_reduce_batch; include/frirl_hip.h, DESIGN.md "Batched reduction").
//
// A round is three launches over the agents that are still reducing (the live list, built on the device):
//   open   slot table of the next d_e = min(depth, R0_e - j_e) candidates of every live agent
//   roll   one replay per node of every live agent's accept/reject tree; a workgroup serves rows of ONE agent and points
//          rollout_episode / shared_sweep (the code of frirl_hip_rollout_shared) at that agent's slab, start state and step cap
//   close  tree walk (reduce_walk.h), in-place compaction of the agent's columns, next live list
// and the host reads one 16-byte header (the live count) per round.  No slab and no per-row result crosses to the host.
// This file holds `roll` and the entry point; the protocol around it (checks, order, open, close, results) is ReduceRun's (reduce_run.h).
#include "rollout_episode.h"
#include "reduce_run.h"
#include "shape_ladder.h"
#include <type_traits>

namespace frirl {

// Batched roll-out kernel: `wpa` workgroups per live agent, each serving 256 / (G * H) nodes of that agent's tree (first: the
// baseline replay, one row per agent, no exclusions).  All conditions in front of the barriers are uniform over the workgroup:
// they depend on the agent and on the workgroup's first row only.
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void reduce_batch_rollout_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                         const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                         const frirl_hip_agent ag, const double *__restrict__ start_states, int cur,
                                                                         int wpa, int first, ReduceBatchWs ws)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int e = ws.live[cur][blockIdx.x / wpa];
    const int row0 = (blockIdx.x % wpa) * EPB;
    const int n = first ? 1 : rw_nodes(ws.d[e]);
    if (row0 >= n) return;                                             // the whole workgroup, before the first barrier
    const int node = row0 + threadIdx.x / GH;
    const bool exists = node < n;                                      // nodes with k >= d_e do not exist
    const uint32_t mask = (exists && !first) ? ws.mask[node] : 0u;
    double states[NS], total;
    int steps, success;
    rollout_episode<NANT, AMAX, G, H, true, KernelPow<NANT, PN>>(tl, grid_s, u, ve, U, rb + (size_t)e * (NANT + 1) * maxR, ws.slot + (size_t)e * maxR, nrules[e], maxR,
                                                                  ag, kernel_pow<NANT, PN>(ag), exists, (uint32_t)node, mask,
                                                                  start_states ? start_states + (size_t)e * NS : nullptr, ws.cap[e], steps, total, success, states);
    if (!exists || threadIdx.x % GH != 0) return;
    ws.steps[(size_t)e * ws.nodes + node] = steps;
    ws.reward[(size_t)e * ws.nodes + node] = total;
}

}  // namespace frirl

extern "C" int frirl_hip_reduce_batch_depth(int32_t E, int32_t A) { return frirl_hip_reduce_batch_starts_depth(E, A, 1); }

extern "C" size_t frirl_hip_reduce_batch_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t depth)
{
    (void)nant;                              // no array of the workspace depends on it
    if (E < 1 || maxR < 1 || depth < 0 || depth > frirl::RW_MAX_DEPTH) return 0;
    if (depth > 0) return reduce_batch_layout(nullptr, E, maxR, depth, (size_t)E * frirl::rw_nodes(depth), nullptr);
    // depth 0: the depth frirl_hip_reduce_batch_depth selects is not known without the action count -- enough for any (the shape of
    // up to 4 actions holds the most rows), and never less for more agents
    const long cap = rb_resident_rows(1);
    return reduce_batch_layout(nullptr, E, maxR, 10, (size_t)((long)E > cap ? (long)E : cap), nullptr);
}

// the replays of the run's current round: one row per node of every live agent
template <int N>
static void launch_rows(const ReduceRun &r, const double *start)
{
    const int nlive = r.nlive(), nodes = r.rows_per_agent(), first = r.first();
    const int H = first ? FRIRL_WAVE / rb_group(r.agent.A) : rb_slices((long)nlive * nodes, r.agent.A);     // the baseline replay: a full wave per row
    frirl::for_batch_shape<N>(&r.agent, H, [&](auto sh) {
        using S = decltype(sh);
        constexpr int EPB = frirl::SH_BLOCK / (S::G * S::H);
        const int wpa = (nodes + EPB - 1) / EPB;
        hipLaunchKernelGGL((frirl::reduce_batch_rollout_kernel<N, S::AMAX, S::G, S::H, S::PN>), dim3((unsigned)nlive * wpa), dim3(frirl::SH_BLOCK), 0, r.s, r.t.u,
                           r.t.ve, r.t.U, r.b.rb, r.b.nrules, r.b.maxR, r.agent, start, r.cur(), wpa, first, r.ws);
    });
}

extern "C" int frirl_hip_reduce_walk_check(int d, const int32_t *steps, const double *reward, int steps_inc, double prev_reward, double good_above,
                                           double tol, uint32_t *bits_out, double *prev_out)
{
    if (d < 0 || d > frirl::RW_MAX_DEPTH || (d > 0 && (!steps || !reward)) || !bits_out || !prev_out) {
        set_error("frirl_hip_reduce_walk_check: d=%d outside 0..%d or NULL argument", d, frirl::RW_MAX_DEPTH);
        return FRIRL_HIP_EINVAL;
    }
    double prev = prev_reward;
    *bits_out = frirl::rw_walk(d, steps, reward, steps_inc, prev, good_above, tol);
    *prev_out = prev;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reduce_batch(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                      const double *start_states, const uint8_t *active, int strategy, double reward_tolerance, int depth,
                                      int32_t *kept, frirl_hip_reduce_result *results, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_reduce_batch";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!agent || !results || !agent->grid_values || !agent->action_ve) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, who)) || (rc = check_grid_len(t, agent, who))) return rc;
    ReduceRun run;
    if ((rc = run.init(who, t, b, agent, rant, nullptr, strategy, reward_tolerance, depth, false, stream)) ||
        (rc = run.check_workspace(who, workspace, workspace_bytes)) || (rc = check_device()) || (rc = run.start(who, workspace, active, nullptr)))
        return rc;
    // round 0 = the baseline replay of every active agent (:196-198 and the first loop iteration, :204-206); then rounds until no
    // agent has a candidate left
    while (run.nlive() > 0) {
        if (t->nant == 3) launch_rows<3>(run, start_states);
        else launch_rows<5>(run, start_states);
        if ((rc = run.close(who))) return rc;
    }
    return run.results(who, kept, results, nullptr);
}
