// reduce_run.hip -- ReduceRun (reduce_run.h): the round protocol of the batched rule-base reductions, written once.  This is the only
// translation unit that holds the order, open, close, result and init kernels (reduce_batch_kernels.h, reduce_starts_kernels.h), so
// every launch of them is here; the three entry points (reduce_batch.hip, reduce_starts.hip, policy_batch.hip) differ only in who runs
// the replays between two calls of close().  Per round the host reads one 16-byte header: the next round's live count.
#include "reduce_run.h"
#include "reduce_starts_kernels.h"
#include "reduce_map_kernels.h"
#include "reduce_orders_kernels.h"

int ReduceRun::init(const char *who, const frirl_hip_tables *t_, const frirl_hip_rulebases *b_, const frirl_hip_agent *agent_, double *rant_,
                    const frirl_hip_reduce_starts *starts, int strategy_, double reward_tolerance_, int depth_, bool stepped_, void *stream)
{
    ns = starts ? starts->n : 0;
    if (starts && (ns < 1 || ns > FRIRL_HIP_REDUCE_MAX_STARTS)) { set_error("%s: n=%d start states outside 1..%d", who, ns, FRIRL_HIP_REDUCE_MAX_STARTS); return FRIRL_HIP_EINVAL; }
    if (strategy_ != 1 && strategy_ != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy_); return FRIRL_HIP_EINVAL; }
    if (depth_ < 0 || depth_ > frirl::RW_MAX_DEPTH) { set_error("%s: depth %d outside 0..%d", who, depth_, frirl::RW_MAX_DEPTH); return FRIRL_HIP_EINVAL; }
    if (agent_->A < 1 || agent_->A > FRIRL_HIP_MAX_ACTIONS || agent_->max_steps < 0) { set_error("%s: A=%d / max_steps=%d out of range", who, agent_->A, agent_->max_steps); return FRIRL_HIP_EINVAL; }
    depth = depth_ ? depth_ : frirl_hip_reduce_batch_starts_depth(b_->E, agent_->A, per_node());
    nodes = frirl::rw_nodes(depth);
    const size_t E = (size_t)b_->E, M = (size_t)b_->maxR, rows = E * per_node() * nodes;
    if (!ns && rows > 0x7fffffffu) { set_error("%s: E=%d agents x %d rows per round beyond 2^31 - 1", who, b_->E, nodes); return FRIRL_HIP_EINVAL; }
    if (ns && rows > (size_t)INT32_MAX / 2) { set_error("%s: E=%d x n=%d x %d nodes: too many rows per round", who, b_->E, ns, nodes); return FRIRL_HIP_EINVAL; }
    t = *t_; b = *b_; agent = *agent_;
    agent.no_random = 1;
    rant = rant_;
    reward_good_above = agent_->reward_good_above;
    reward_tolerance = reward_tolerance_;
    strategy = strategy_;
    drop_bad = starts && starts->drop_bad_starts != 0;
    stepped = stepped_;
    need = ns ? reduce_starts_layout(nullptr, E, M, depth, rows, ns, nullptr) : reduce_batch_layout(nullptr, E, M, depth, rows, nullptr);
    s = as_stream(stream);
    return FRIRL_HIP_OK;
}

int ReduceRun::check_workspace(const char *who, const void *workspace, size_t bytes) const
{
    if (workspace && !(reinterpret_cast<uintptr_t>(workspace) & 15) && bytes >= need) return FRIRL_HIP_OK;
    set_error("%s: workspace %p / %zu bytes: needs %zu bytes, 16-byte aligned (%s)", who, workspace, bytes, need,
              ns ? "frirl_hip_reduce_batch_starts_workspace_bytes" : "frirl_hip_reduce_batch_workspace_bytes");
    return FRIRL_HIP_EINVAL;
}

int ReduceRun::start(const char *who, void *workspace, const uint8_t *active, const int32_t *start_count)
{
    const size_t E = (size_t)b.E, M = (size_t)b.maxR, rows = E * per_node() * nodes;
    if (ns) {
        reduce_starts_layout(static_cast<char *>(workspace), E, M, depth, rows, ns, &sw);
        ws = sw.b;
    } else {
        reduce_batch_layout(static_cast<char *>(workspace), E, M, depth, rows, &ws);
    }
    round = 0;
    // round 0 appends to list 1 without an open kernel before it: the header is zeroed here; later rounds zero the other count in `open`
    FRIRL_HIP_TRY(hipMemsetAsync(ws.hdr, 0, sizeof hdr, s), who, return FRIRL_HIP_ELAUNCH);
    hipLaunchKernelGGL(frirl::reduce_batch_order_kernel, dim3((unsigned)E), dim3(256), 0, s, b.rb, b.nrules, t.nant, b.maxR, active, strategy, agent.max_steps,
                       ws);
    if (ns) hipLaunchKernelGGL(frirl::reduce_starts_init_kernel, dim3((unsigned)E), dim3(256), 0, s, start_count, sw);
    int rc = header(who);
    if (rc || (rc = check_launch(who))) return rc;
    if (hdr[2]) { set_error("%s: agent %d: nrules outside 1..maxR=%d", who, hdr[2] - 1, b.maxR); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

int ReduceRun::header(const char *who)
{
    FRIRL_HIP_TRY(hipMemcpyAsync(hdr, ws.hdr, sizeof hdr, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    return FRIRL_HIP_OK;
}

// the three kinds of close kernel: one row per node, nodes x starts in compact rows, nodes x starts in the caller-stepped rows
template <int N>
static void launch_close(const ReduceRun &r)
{
    const dim3 grid(r.nlive()), block(256);
    const int cur = r.cur(), first = r.first(), maxR = r.b.maxR, max_steps = r.agent.max_steps;
    if (!r.ns)
        hipLaunchKernelGGL(frirl::reduce_batch_close_kernel<N>, grid, block, 0, r.s, r.b.rb, r.b.nrules, r.b.uidx, r.rant, maxR, cur, first, max_steps,
                           r.reward_good_above, r.reward_tolerance, r.ws);
    else if (r.stepped)
        hipLaunchKernelGGL((frirl::reduce_starts_close_kernel<N, true>), grid, block, 0, r.s, r.b.rb, r.b.nrules, r.b.uidx, r.rant, maxR, cur, first, max_steps,
                           r.reward_good_above, r.reward_tolerance, r.drop_bad, r.sw);
    else if constexpr (N == 3 || N == 5)                              // compact rows come from the demo roll-outs: 3 or 5 antecedents
        hipLaunchKernelGGL((frirl::reduce_starts_close_kernel<N, false>), grid, block, 0, r.s, r.b.rb, r.b.nrules, r.b.uidx, r.rant, maxR, cur, first, max_steps,
                           r.reward_good_above, r.reward_tolerance, r.drop_bad, r.sw);
}

int ReduceRun::close(const char *who)
{
    switch (t.nant) {
#define M(N) case N: launch_close<N>(*this); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
    const int rc = header(who);                                       // the next round's live count
    if (rc) return rc;
    round += 1;
    if (nlive() > 0) hipLaunchKernelGGL(frirl::reduce_batch_open_kernel, dim3(nlive()), dim3(256), 0, s, b.nrules, b.maxR, depth, cur(), ws);
    return check_launch(who);
}

int ReduceRun::results(const char *who, int32_t *kept, frirl_hip_reduce_result *results, frirl_hip_reduce_start_result *per_start)
{
    const size_t E = (size_t)b.E, M = (size_t)b.maxR, total = E * ns;
    if (results) hipLaunchKernelGGL(frirl::reduce_batch_result_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, b.nrules, (int)E, ws);
    if (per_start) hipLaunchKernelGGL(frirl::reduce_starts_result_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (int)total, sw);
    if (results) FRIRL_HIP_TRY(hipMemcpyAsync(results, ws.res, sizeof(frirl_hip_reduce_result) * E, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    if (per_start) FRIRL_HIP_TRY(hipMemcpyAsync(per_start, sw.res, sizeof(frirl_hip_reduce_start_result) * total, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    if (kept) FRIRL_HIP_TRY(hipMemcpyAsync(kept, ws.alive, sizeof(int32_t) * E * M, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    return check_launch(who);
}

// ---- the map-validated reduction (frirl_hip_reduce_batch_map, policy_map.hip): its launches of the order kernel and of the kernel that
// reuses the compaction sit in this translation unit (reduce_map_ws.h) ----
int reduce_map_launch_order(const char *who, const frirl_hip_tables &t, const frirl_hip_rulebases &b, const uint8_t *active, int strategy,
                            const ReduceMapWs &ws, hipStream_t s)
{
    FRIRL_HIP_TRY(hipMemsetAsync(ws.b.hdr, 0, 4 * sizeof(int32_t), s), who, return FRIRL_HIP_ELAUNCH);
    hipLaunchKernelGGL(frirl::reduce_batch_order_kernel, dim3((unsigned)b.E), dim3(256), 0, s, b.rb, b.nrules, t.nant, b.maxR, active, strategy, 0, ws.b);
    return check_launch(who);
}

template <int N>
static void launch_reduce_map(const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident, const ReduceMapWs &ws, hipStream_t s)
{
    const int rcap = resident ? frirl::map_resident_rules(N, b.maxR) : 0;
    const size_t lds = (size_t)rcap * frirl::map_rule_bytes(N);
    // one action per lane while every (point, action) pair of an agent fits one pass of its workgroup, else blocks of 4
    if ((long)m.n * m.A <= frirl::PM_BLOCK)
        hipLaunchKernelGGL((frirl::reduce_map_kernel<N, 1>), dim3((unsigned)b.E), dim3(frirl::PM_BLOCK), lds, s, b.rb, b.nrules, b.uidx, rant, b.maxR, m, rcap, ws);
    else
        hipLaunchKernelGGL((frirl::reduce_map_kernel<N, 4>), dim3((unsigned)b.E), dim3(frirl::PM_BLOCK), lds, s, b.rb, b.nrules, b.uidx, rant, b.maxR, m, rcap, ws);
}

void reduce_map_launch_run(const frirl_hip_tables &t, const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident,
                           const ReduceMapWs &ws, hipStream_t s)
{
    switch (t.nant) {
#define M(N) case N: launch_reduce_map<N>(b, rant, m, resident, ws, s); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
}

// ---- the map-validated reduction over several orders (frirl_hip_reduce_batch_map_orders, policy_map.hip): its kernels reuse the
// compaction, so their launches sit in this translation unit too (reduce_orders_ws.h) ----
int reduce_orders_launch_check(const char *who, const frirl_hip_rulebases &b, const frirl::MapArgs &m, int nant, const int32_t *orders,
                               const ReduceOrdersWs &ws, hipStream_t s)
{
    FRIRL_HIP_TRY(hipMemsetAsync(ws.hdr, 0, 4 * sizeof(int32_t), s), who, return FRIRL_HIP_ELAUNCH);
    hipLaunchKernelGGL(frirl::reduce_orders_check_kernel, dim3((unsigned)b.E * (unsigned)ws.K), dim3(256), 0, s, b.nrules, b.maxR, m, nant - 1, orders, ws);
    return check_launch(who);
}

template <int N>
static void launch_reduce_orders(const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident, const int32_t *orders,
                                 const ReduceOrdersWs &ws, hipStream_t s)
{
    const int rcap = resident ? frirl::map_resident_rules(N, b.maxR) : 0;
    const size_t lds = (size_t)rcap * frirl::map_rule_bytes(N);
    const dim3 grid((unsigned)b.E * (unsigned)ws.K), block(frirl::PM_BLOCK);
    // reduce_map_kernel's lane shapes: one action per lane while an agent's (point, action) pairs fit one pass, else blocks of 4
    if ((long)m.n * m.A <= frirl::PM_BLOCK)
        hipLaunchKernelGGL((frirl::reduce_orders_trial_kernel<N, 1>), grid, block, lds, s, b.rb, b.nrules, b.maxR, m, rcap, orders, ws);
    else
        hipLaunchKernelGGL((frirl::reduce_orders_trial_kernel<N, 4>), grid, block, lds, s, b.rb, b.nrules, b.maxR, m, rcap, orders, ws);
    hipLaunchKernelGGL(frirl::reduce_orders_apply_kernel<N>, dim3((unsigned)b.E), dim3(256), 0, s, b.rb, b.nrules, b.uidx, rant, b.maxR, m, ws);
}

void reduce_orders_launch_run(const frirl_hip_tables &t, const frirl_hip_rulebases &b, double *rant, const frirl::MapArgs &m, int resident,
                              const int32_t *orders, const ReduceOrdersWs &ws, hipStream_t s)
{
    switch (t.nant) {
#define M(N) case N: launch_reduce_orders<N>(b, rant, m, resident, orders, ws, s); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
}
