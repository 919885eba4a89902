// reduce_starts.hip -- frirl_hip_reduce_batch (reduce_batch.hip) with every removal validated against SEVERAL start states per agent
// (frirl_hip_reduce_batch_starts; include/frirl_hip.h, DESIGN.md "Reduction against a set of start states").
//
// The order, open-round and result kernels, the masks, the slot tables, the live lists and the compaction are those of the batched
// reduction (reduce_batch_kernels.h).  New here: a row space of nodes x used starts per agent (row = node * K_e + ki), per-start
// baselines and step caps, and a close kernel that accepts a removal only if every used start accepts it (rw_walk_starts).  The
// per-start arrays, the init, close and result kernels and the layout are reduce_starts_kernels.h (shared with the caller-stepped form).
//   roll   a workgroup serves 256 / (G * H) rows of ONE agent; rows with different caps share it, so the step loop is written here:
//          its bound is the agent's largest cap, a row goes inactive after its own cap, the workgroup leaves through
//          __syncthreads_count.  Per row the result is rollout_episode's (rollout_episode.h) with max_steps = the row's cap.
//   close  first: per-start baselines, caps and the compact list of used starts; otherwise walk, compaction, next live list.
#include "shared_sweep.h"
#include "envs.h"
#include "reduce_starts_kernels.h"
#include "shape_ladder.h"

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
    using POW = typename std::conditional<PN, PowC<NANT>, PowU>::type;
    POW p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;

    // ---- rollout_episode's body with the row's own cap inside a loop whose bound is uniform ----
    const int gl = threadIdx.x % GH, sub = gl % G, h = gl / G;        // group lane = (rule slice h, action slot sub)
    const int apl = (ag.A + G - 1) / G;                                // actions per lane
    const int abeg = (sub * apl < ag.A) ? sub * apl : ag.A;
    const int aend = (abeg + apl < ag.A) ? abeg + apl : ag.A;
    const int nchunks = (apl + AMAX - 1) / AMAX;
    for (int i = threadIdx.x; i < NANT * FRIRL_HIP_MAX_GRID; i += SH_BLOCK) grid_s[i] = ag.grid_values[i];
    if ((int)threadIdx.x < ag.A) tl.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
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
    if (!exists || gl != 0) return;
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

template <int N, int AMAX, int G, int H, bool PN = true>
static void launch_rows(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const double *start, int cur, int nlive,
                        int rows, int first, const ReduceStartsWs &ws, hipStream_t s)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    const int wpa = (rows + EPB - 1) / EPB;
    hipLaunchKernelGGL((frirl::reduce_starts_rollout_kernel<N, AMAX, G, H, PN>), dim3((unsigned)nlive * wpa), dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb,
                       b->nrules, b->maxR, *ag, start, cur, wpa, first, ws);
}

// rows: the most rows an agent can have this round (n baseline replays, or nodes * n)
template <int N>
static void launch_rows_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const double *start, int cur, int nlive,
                          int rows, int first, const ReduceStartsWs &ws, hipStream_t s)
{
    const int H = (first && ws.n == 1) ? FRIRL_WAVE / rb_group(ag->A) : rb_slices((long)nlive * rows, ag->A);   // one baseline replay per agent: a full wave per row
    frirl::for_batch_shape<N>(ag, H, [&](auto sh) {
        using S = decltype(sh);
        launch_rows<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, start, cur, nlive, rows, first, ws, s);
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
    if (starts->n < 1 || starts->n > FRIRL_HIP_REDUCE_MAX_STARTS) { set_error("%s: n=%d start states outside 1..%d", who, starts->n, FRIRL_HIP_REDUCE_MAX_STARTS); return FRIRL_HIP_EINVAL; }
    if (strategy != 1 && strategy != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy); return FRIRL_HIP_EINVAL; }
    if (depth < 0 || depth > frirl::RW_MAX_DEPTH) { set_error("%s: depth %d outside 0..%d", who, depth, frirl::RW_MAX_DEPTH); return FRIRL_HIP_EINVAL; }
    if (agent->A < 1 || agent->A > FRIRL_HIP_MAX_ACTIONS || agent->max_steps < 0) { set_error("%s: A=%d / max_steps=%d out of range", who, agent->A, agent->max_steps); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, who))) return rc;
    if ((rc = check_grid_len(t, agent, who))) return rc;
    const int n = starts->n, drop_bad = starts->drop_bad_starts != 0;
    if (depth == 0) depth = frirl_hip_reduce_batch_starts_depth(b->E, agent->A, n);
    const size_t E = (size_t)b->E, M = (size_t)b->maxR;
    const int nodes = frirl::rw_nodes(depth);
    if (E * n * nodes > (size_t)INT32_MAX / 2) { set_error("%s: E=%zu x n=%d x %d nodes: too many rows per round", who, E, n, nodes); return FRIRL_HIP_EINVAL; }
    const size_t need = reduce_starts_layout(nullptr, E, M, depth, E * n * nodes, n, nullptr);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need) {
        set_error("%s: workspace %p / %zu bytes: needs %zu bytes, 16-byte aligned (frirl_hip_reduce_batch_starts_workspace_bytes)", who, workspace, workspace_bytes, need);
        return FRIRL_HIP_EINVAL;
    }
    if ((rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
#define RS_TRY(expr)                                                                                               \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) { set_error("%s: %s: %s", who, #expr, hipGetErrorString(e_)); return FRIRL_HIP_ELAUNCH; } \
    } while (0)
    ReduceStartsWs ws;
    reduce_starts_layout(static_cast<char *>(workspace), E, M, depth, E * n * nodes, n, &ws);
    frirl_hip_agent greedy = *agent;
    greedy.no_random = 1;                                             // the replays are greedy, as frirl_hip_reduce_batch forces it
    int32_t hdr[4] = {0, 0, 0, 0};
    RS_TRY(hipMemsetAsync(ws.b.hdr, 0, sizeof hdr, s));
    hipLaunchKernelGGL(frirl::reduce_batch_order_kernel, dim3((unsigned)E), dim3(256), 0, s, b->rb, b->nrules, t->nant, b->maxR, active, strategy,
                       greedy.max_steps, ws.b);
    hipLaunchKernelGGL(frirl::reduce_starts_init_kernel, dim3((unsigned)E), dim3(256), 0, s, starts->start_count, ws);
    RS_TRY(hipMemcpyAsync(hdr, ws.b.hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
    RS_TRY(hipStreamSynchronize(s));
    if (hdr[2]) { set_error("%s: agent %d: nrules outside 1..maxR=%d", who, hdr[2] - 1, b->maxR); return FRIRL_HIP_EINVAL; }
    // round 0 = the baseline replays of every active agent; then rounds until no agent has a candidate left.  Per round the host reads
    // the 16-byte header: the next round's live count.
    for (int round = 0;; round++) {
        const int cur = round & 1, first = round == 0;
        const int nlive = hdr[cur];
        if (nlive == 0) break;
        // round 0 appends to list 1 without an open kernel before it: the header was zeroed above; later rounds zero the other count here
        if (!first) hipLaunchKernelGGL(frirl::reduce_batch_open_kernel, dim3(nlive), dim3(256), 0, s, b->nrules, b->maxR, depth, cur, ws.b);
        const int rows = first ? n : nodes * n;
        if (t->nant == 3) launch_rows_n<3>(t, b, &greedy, starts->start_states, cur, nlive, rows, first, ws, s);
        else launch_rows_n<5>(t, b, &greedy, starts->start_states, cur, nlive, rows, first, ws, s);
        if (t->nant == 3)
            hipLaunchKernelGGL(frirl::reduce_starts_close_kernel<3>, dim3(nlive), dim3(256), 0, s, b->rb, b->nrules, b->uidx, rant, b->maxR, cur, first,
                               greedy.max_steps, agent->reward_good_above, reward_tolerance, drop_bad, ws);
        else
            hipLaunchKernelGGL(frirl::reduce_starts_close_kernel<5>, dim3(nlive), dim3(256), 0, s, b->rb, b->nrules, b->uidx, rant, b->maxR, cur, first,
                               greedy.max_steps, agent->reward_good_above, reward_tolerance, drop_bad, ws);
        RS_TRY(hipMemcpyAsync(hdr, ws.b.hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
        RS_TRY(hipStreamSynchronize(s));
    }
    hipLaunchKernelGGL(frirl::reduce_batch_result_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, b->nrules, (int)E, ws.b);
    hipLaunchKernelGGL(frirl::reduce_starts_result_kernel, dim3((unsigned)((E * n + 255) / 256)), dim3(256), 0, s, (int)(E * n), ws);
    RS_TRY(hipMemcpyAsync(results, ws.b.res, sizeof(frirl_hip_reduce_result) * E, hipMemcpyDeviceToHost, s));
    if (per_start) RS_TRY(hipMemcpyAsync(per_start, ws.res, sizeof(frirl_hip_reduce_start_result) * E * n, hipMemcpyDeviceToHost, s));
    if (kept) RS_TRY(hipMemcpyAsync(kept, ws.b.alive, sizeof(int32_t) * E * M, hipMemcpyDeviceToHost, s));
    RS_TRY(hipStreamSynchronize(s));
#undef RS_TRY
    return check_launch(who);
}
