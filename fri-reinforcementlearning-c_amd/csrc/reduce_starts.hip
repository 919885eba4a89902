// reduce_starts.hip -- frirl_hip_reduce_batch (reduce_batch.hip) with every removal validated against SEVERAL start states per agent
// (frirl_hip_reduce_batch_starts; include/frirl_hip.h, DESIGN.md "Reduction against a set of start states").
//
// The round protocol is ReduceRun's (reduce_run.h), as for frirl_hip_reduce_batch; with start states it adds the init kernel and a
// close kernel that accepts a removal only if every used start accepts it (rw_walk_starts).  This file holds the entry point and
//   roll   a row space of nodes x used starts per agent (row = node * K_e + ki) with per-start baselines and step caps (ReduceStartsWs,
//          reduce_ws.h).  A workgroup serves 256 / (G * H) rows of ONE agent; rows with different caps share it, so the step loop is
//          written here: its bound is the agent's largest cap, a row goes inactive after its own cap, the workgroup leaves through
//          __syncthreads_count.  Per row the result is rollout_episode's (rollout_episode.h) with max_steps = the row's cap.
#include "shared_sweep.h"
#include "envs.h"
#include "reduce_run.h"
#include "shape_ladder.h"
#include <type_traits>

namespace frirl {

// Roll-out kernel: `wpa` workgroups per live agent, each serving 256 / (G * H) rows of that agent.  first: the baseline replays, row k
// = start k, no exclusions, cap max_steps.  Otherwise row r = node * K_e + ki: the node's mask, the ki-th used start and that start's
// cap.  All conditions in front of the barriers depend on the agent and on the workgroup's first row only.
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void reduce_starts_rollout_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                          const double *__restrict__ rb_all, const int32_t *__restrict__ nrules, int maxR,
                                                                          const frirl_hip_agent ag, const double *__restrict__ start_states, int cur,
                                                                          int wpa, int first, ReduceStartsWs ws)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int e = ws.b.live[cur][blockIdx.x / wpa];
    const int row0 = (blockIdx.x % wpa) * EPB;
    const int Ke = first ? ws.cnt[e] : ws.K[e];
    const int rows = first ? Ke : rw_nodes(ws.b.d[e]) * Ke;
    if (row0 >= rows) return;                                          // the whole workgroup, before the first barrier
    const int bound = first ? ag.max_steps : ws.capmax[e];             // uniform: the agent's largest cap
    const int r = row0 + threadIdx.x / GH;
    const bool exists = r < rows;
    const size_t en = (size_t)e * ws.n;
    int node = 0, k = 0, cap = 0;
    if (exists) {
        node = r / Ke;
        k = r - node * Ke;
        if (!first) k = ws.used[en + k];
        cap = first ? ag.max_steps : ws.cap[en + k];
    }
    const uint32_t mask = (exists && !first) ? ws.b.mask[node] : 0u;
    const double *start = start_states + (en + k) * NS;
    const double *rb = rb_all + (size_t)e * (NANT + 1) * maxR;
    const uint8_t *slot_g = ws.b.slot + (size_t)e * maxR;
    const int R = nrules[e];
    using POW = KernelPow<NANT, PN>;
    const POW p = kernel_pow<NANT, PN>(ag);

    // ---- rollout_episode's body with the row's own cap inside a loop whose bound is uniform (why it is not a call of
    // rollout_episode: profiles/r24_rollout_loop.md, "tried and put aside") ----
    const GroupLane l = group_lane<G, H, AMAX>(ag.A);
    const int abeg = l.abeg, aend = l.aend, nchunks = l.nchunks, h = l.h;
    stage_agent<NANT>(tl, grid_s, ag);
    double states[NS], cs[NS], qs[NS], q[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        states[i] = exists ? start[i] : ag.values_def[i];                                                // frirl_episode.c:46-48
        q[i] = observe_ve(u, ve, U, i, states[i]);
    }
    unsigned h0;
    int a;
    double bv;
    shared_sweep<NANT, AMAX, true, true, G, H, POW>(tl, rb, slot_g, R, maxR, p, abeg, aend, nchunks, q, exists, mask, nullptr, h0, a, bv, h);   // :78
    group_first_max<G>(bv, a);
    a = e_greedy(ag, a, (uint32_t)r, 0u, 0u);
    double action = grid_s[NS * FRIRL_HIP_MAX_GRID + a];                                                 // :82
    int steps = 0, success = 0;
    double total = 0.0;
    bool active = exists && cap > 0;
    for (int step = 1; step <= bound; step++) {                                                          // :86
        if (__syncthreads_count(active ? 1 : 0) == 0) break;                                             // every row's episode has ended
        if (active) {
            double rw;
            env_do_action(ag.env_kind, action, states, cs);                                              // :97
            env_get_reward(ag.env_kind, cs, rw, success);                                                // :106
            total = total + rw;                                                                          // :107
            env_quantize(ag.env_kind, NS, grid_s, ag.grid_len, ag.grid_div, cs, qs);                     // :112
#pragma unroll
            for (int i = 0; i < NS; i++) q[i] = observe_ve(u, ve, U, i, qs[i]);
        }
        int pa;
        shared_sweep<NANT, AMAX, true, true, G, H, POW>(tl, rb, slot_g, R, maxR, p, abeg, aend, nchunks, q, active, mask, nullptr, h0, pa, bv, h);   // :148
        group_first_max<G>(bv, pa);
        if (active) {
            pa = e_greedy(ag, pa, (uint32_t)r, 0u, (uint32_t)step);
            action = grid_s[NS * FRIRL_HIP_MAX_GRID + pa];                                               // :151
#pragma unroll
            for (int i = 0; i < NS; i++) states[i] = cs[i];                                              // :163-165
            steps++;                                                                                     // :174
            if (success == 1 || steps >= cap) active = false;                                            // :183; :86 with the row's cap
        }
    }
    if (!exists || !l.leader) return;
    const size_t out = (size_t)e * ws.b.nodes * ws.n + r;
    ws.b.steps[out] = steps;
    ws.b.reward[out] = total;
}

}  // namespace frirl

extern "C" int frirl_hip_reduce_batch_starts_depth(int32_t E, int32_t A, int32_t n)
{
    if (E < 1) E = 1;
    if (n < 1) n = 1;
    const long rows = rb_resident_rows(A);
    int d = 1;
    while (d < 10 && (long)E * n * frirl::rw_nodes(d + 1) <= rows) d++;
    return d;
}

extern "C" size_t frirl_hip_reduce_batch_starts_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t depth, int32_t n)
{
    (void)nant;                              // no array of the workspace depends on it
    if (E < 1 || maxR < 1 || depth < 0 || depth > frirl::RW_MAX_DEPTH || n < 1 || n > FRIRL_HIP_REDUCE_MAX_STARTS) return 0;
    if (depth > 0) return reduce_starts_layout(nullptr, E, maxR, depth, (size_t)E * n * frirl::rw_nodes(depth), n, nullptr);
    // depth 0: enough for whatever depth the rule selects, for any action count (as frirl_hip_reduce_batch_workspace_bytes)
    const long cap = rb_resident_rows(1), en = (long)E * n;
    return reduce_starts_layout(nullptr, E, maxR, 10, (size_t)(en > cap ? en : cap), n, nullptr);
}

// the replays of the run's current round; rows: the most rows an agent can have this round (n baseline replays, or nodes * n)
template <int N>
static void launch_rows(const ReduceRun &r, const double *start)
{
    const int nlive = r.nlive(), rows = r.rows_per_agent(), first = r.first();
    const int H = (first && r.ns == 1) ? FRIRL_WAVE / rb_group(r.agent.A) : rb_slices((long)nlive * rows, r.agent.A);   // one baseline replay per agent: a full wave per row
    frirl::for_batch_shape<N>(&r.agent, H, [&](auto sh) {
        using S = decltype(sh);
        constexpr int EPB = frirl::SH_BLOCK / (S::G * S::H);
        const int wpa = (rows + EPB - 1) / EPB;
        hipLaunchKernelGGL((frirl::reduce_starts_rollout_kernel<N, S::AMAX, S::G, S::H, S::PN>), dim3((unsigned)nlive * wpa), dim3(frirl::SH_BLOCK), 0, r.s, r.t.u,
                           r.t.ve, r.t.U, r.b.rb, r.b.nrules, r.b.maxR, r.agent, start, r.cur(), wpa, first, r.sw);
    });
}

extern "C" int frirl_hip_reduce_walk_starts_check(int d, int K, const int32_t *steps, const double *reward, const int32_t *steps_inc, double *prev,
                                                  double good_above, double tol, uint32_t *bits_out)
{
    if (d < 0 || d > frirl::RW_MAX_DEPTH || K < 1 || K > FRIRL_HIP_REDUCE_MAX_STARTS || (d > 0 && (!steps || !reward)) || !steps_inc || !prev || !bits_out) {
        set_error("frirl_hip_reduce_walk_starts_check: d=%d outside 0..%d, K=%d outside 1..%d or NULL argument", d, frirl::RW_MAX_DEPTH, K,
                  FRIRL_HIP_REDUCE_MAX_STARTS);
        return FRIRL_HIP_EINVAL;
    }
    *bits_out = frirl::rw_walk_starts(d, K, K, false, steps, reward, nullptr, steps_inc, prev, good_above, tol);
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reduce_walk_starts_rows_check(int d, int K, int n, const int32_t *used, const int32_t *steps, const double *reward,
                                                       const int32_t *steps_inc, double *prev, double good_above, double tol, uint32_t *bits_out)
{
    bool ok = d >= 0 && d <= frirl::RW_MAX_DEPTH && n >= 1 && n <= FRIRL_HIP_REDUCE_MAX_STARTS && K >= 1 && K <= n && used && (d == 0 || (steps && reward)) &&
              steps_inc && prev && bits_out;
    for (int ki = 0; ok && ki < K; ki++) ok = used[ki] >= 0 && used[ki] < n;
    if (!ok) {
        set_error("frirl_hip_reduce_walk_starts_rows_check: d=%d outside 0..%d, n=%d outside 1..%d, K=%d outside 1..n, used[] outside 0..n-1 or NULL argument", d,
                  frirl::RW_MAX_DEPTH, n, FRIRL_HIP_REDUCE_MAX_STARTS, K);
        return FRIRL_HIP_EINVAL;
    }
    *bits_out = frirl::rw_walk_starts(d, K, n, true, steps, reward, used, steps_inc, prev, good_above, tol);
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reduce_batch_starts(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                             const frirl_hip_reduce_starts *starts, const uint8_t *active, int strategy, double reward_tolerance,
                                             int depth, int32_t *kept, frirl_hip_reduce_result *results, frirl_hip_reduce_start_result *per_start,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_reduce_batch_starts";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!agent || !results || !starts || !starts->start_states || !agent->grid_values || !agent->action_ve) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, who)) || (rc = check_grid_len(t, agent, who))) return rc;
    ReduceRun run;
    if ((rc = run.init(who, t, b, agent, rant, starts, strategy, reward_tolerance, depth, false, stream)) ||
        (rc = run.check_workspace(who, workspace, workspace_bytes)) || (rc = check_device()) ||
        (rc = run.start(who, workspace, active, starts->start_count)))
        return rc;
    // round 0 = the baseline replays of every active agent; then rounds until no agent has a candidate left
    while (run.nlive() > 0) {
        if (t->nant == 3) launch_rows<3>(run, starts->start_states);
        else launch_rows<5>(run, starts->start_states);
        if ((rc = run.close(who))) return rc;
    }
    return run.results(who, kept, results, per_start);
}
