// policy_map.hip -- what a rule base does at a set of points (include/frirl_hip.h): the map kernel and entry point
// (frirl_hip_policy_map), the entry point of the reduction validated on the map (frirl_hip_reduce_batch_map; its kernel sits behind
// reduce_map_ws.h, beside the order kernel and the compaction it reuses), of the same reduction over several caller orders
// (frirl_hip_reduce_batch_map_orders; kernels behind reduce_orders_ws.h) and the points of recorded roll-outs (frirl_hip_log_points).
#include "reduce_orders_ws.h"

namespace frirl {

// Map kernel: workgroup (e, g) serves the points [g * ppp, (g + 1) * ppp) of agent e in one pass (policy_map_sweep.h).  All conditions
// in front of the barriers are uniform over the workgroup.
template <int NANT, int AMAX>
__global__ __launch_bounds__(PM_BLOCK) void policy_map_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR, const MapArgs m,
                                                               int groups, int rcap, double *qve_all, int32_t *__restrict__ best,
                                                               double *__restrict__ actconc)
{
    constexpr int NS = NANT - 1;
    extern __shared__ double lds_rules[];                              // [NANT + 1][rcap] columns
    __shared__ MapPassLds pl;
    __shared__ double ave[FRIRL_HIP_MAX_ACTIONS];
    const int e = blockIdx.x / groups, g = blockIdx.x - e * groups, tid = threadIdx.x;
    const MapShape shape = map_shape(m.A, AMAX);
    const int pt0 = g * shape.ppp;
    const int R = nrules[e];
    const bool ok = (!m.active || m.active[e] != 0) && R >= 1 && R <= maxR;
    int cnt = m.point_count ? m.point_count[e] : m.n;
    cnt = cnt < 0 ? 0 : (cnt > m.n ? m.n : cnt);
    if (!ok) cnt = 0;
    const int my = tid / shape.chunks, pt = pt0 + my;
    const bool first = tid - my * shape.chunks == 0 && my < shape.ppp && pt < m.n;       // the lane that answers for point pt
    if (first && pt >= cnt) best[(size_t)e * m.n + pt] = -1;
    if (pt0 >= cnt) return;
    const size_t M = (size_t)maxR;
    const double *cols_g = rb + (size_t)e * (NANT + 1) * M;
    double *qve = qve_all + (size_t)e * m.n * NS;
    const double *pts = m.points + (size_t)e * m.n * NS;
    const int last = pt0 + shape.ppp < cnt ? pt0 + shape.ppp : cnt;
    for (int i = pt0 * NS + tid; i < last * NS; i += PM_BLOCK) qve[i] = observe_ve(m.u, m.ve, m.U, i % NS, pts[i]);
    if (tid < m.A) ave[tid] = m.action_ve[tid];
    const bool resident = R <= rcap;
    if (resident) map_stage<NANT>(lds_rules, rcap, cols_g, M, R);
    __syncthreads();
    double *conc = actconc ? actconc + (size_t)e * m.n * m.A : nullptr;
    const PowU pw{m.p};
    const int b = resident ? map_pass<NANT, AMAX>(pl, lds_rules, (size_t)rcap, nullptr, R, -1, pw, ave, m.A, shape, qve, pt0, cnt, conc)
                           : map_pass<NANT, AMAX>(pl, cols_g, M, nullptr, R, -1, pw, ave, m.A, shape, qve, pt0, cnt, conc);
    if (b >= 0) best[(size_t)e * m.n + pt] = b;
}

constexpr int LP_BLOCK = 256;

// Which records of a log contribute: one workgroup per log.  The thread of an episode's LAST record (the record before the next start
// record, or the last record written) walks the episode back to its start record and marks every record of it.
__global__ __launch_bounds__(LP_BLOCK) void log_points_mark_kernel(const frirl_hip_log_points_desc lp, uint8_t *__restrict__ take_all)
{
    const size_t q = blockIdx.x;
    int len = lp.length[q];
    len = len < 0 ? 0 : (len > lp.T ? lp.T : len);
    const uint8_t *start = lp.start + q * lp.T;
    uint8_t *take = take_all + q * lp.T;
    for (int r = threadIdx.x; r < len; r += LP_BLOCK) {
        if (r + 1 < len && !start[r + 1]) continue;                    // not the last record of its episode
        const uint8_t v = (!lp.only_successful || lp.success[q * lp.T + r] == 1) ? 1 : 0;
        for (int i = r; i >= 0; i--) {
            take[i] = v;
            if (start[i]) break;
        }
    }
}

// De-duplication: one workgroup per agent.  The candidates (log ascending, record ascending) are taken 256 at a time: a thread's
// candidate is new iff it contributes, no point of the list so far equals it bit-wise and no EARLIER contributing candidate of the chunk
// does; the new ones are appended in candidate order.  Once the list is full any new point raises `overflow`.
template <int NS>
__global__ __launch_bounds__(LP_BLOCK) void log_points_dedup_kernel(const frirl_hip_log_points_desc lp, const uint8_t *__restrict__ take_all)
{
    __shared__ uint64_t cand[LP_BLOCK][NS];
    __shared__ uint8_t ctake[LP_BLOCK];
    __shared__ int wave_new[LP_BLOCK / FRIRL_WAVE];
    const int e = blockIdx.x, tid = threadIdx.x;
    const long N = (long)lp.n_logs * lp.T;
    const size_t q0 = (size_t)e * lp.n_logs;
    uint64_t *list = reinterpret_cast<uint64_t *>(lp.points) + (size_t)e * lp.cap * NS;
    int count = 0, over = 0;                                           // the same in every thread
    for (long c0 = 0; c0 < N; c0 += LP_BLOCK) {
        const long c = c0 + tid;
        uint64_t x[NS] = {};
        bool mine = false;
        if (c < N) {
            const size_t rec = q0 * lp.T + (size_t)c;                  // logs of one agent are contiguous: (j, record) = (c / T, c % T)
            int len = lp.length[q0 + c / lp.T];
            mine = (int)(c % lp.T) < len && take_all[rec] != 0;
            if (mine) {
                const uint64_t *src = reinterpret_cast<const uint64_t *>(lp.start[rec] ? lp.obs : lp.q_obs) + rec * NS;
#pragma unroll
                for (int k = 0; k < NS; k++) x[k] = src[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NS; k++) cand[tid][k] = mine ? x[k] : 0;
        ctake[tid] = mine ? 1 : 0;
        __syncthreads();                                               // also: the list rows written for the last chunk are visible
        bool fresh = mine;
        for (int i = 0; fresh && i < count; i++) {
            bool same = true;
#pragma unroll
            for (int k = 0; k < NS; k++) same = same && list[(size_t)i * NS + k] == x[k];
            fresh = !same;
        }
        for (int i = 0; fresh && i < tid; i++) {
            bool same = ctake[i] != 0;
#pragma unroll
            for (int k = 0; k < NS; k++) same = same && cand[i][k] == x[k];
            fresh = !same;
        }
        const int pos = block_append<LP_BLOCK>(fresh, wave_new, lp.cap, count, over);
        if (fresh && pos < lp.cap) {
#pragma unroll
            for (int k = 0; k < NS; k++) list[(size_t)pos * NS + k] = x[k];
        }
        __syncthreads();                                              // cand / ctake / wave_new are rewritten by the next chunk
    }
    if (tid == 0) { lp.point_count[e] = count; lp.overflow[e] = over; }
}

}  // namespace frirl

extern "C" size_t frirl_hip_policy_map_workspace_bytes(int32_t nant, int32_t E, int32_t n)
{
    if (nant < 2 || E < 1 || n < 1) return 0;
    return up16(sizeof(double) * (size_t)E * (size_t)n * (size_t)(nant - 1));
}

extern "C" size_t frirl_hip_reduce_batch_map_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t n)
{
    if (nant < 2 || E < 1 || maxR < 1 || n < 1) return 0;
    return reduce_map_layout(nullptr, (size_t)E, (size_t)maxR, (size_t)n, nant, nullptr);
}

extern "C" size_t frirl_hip_reduce_batch_map_orders_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t n, int32_t K)
{
    if (nant < 2 || E < 1 || maxR < 1 || n < 1 || K < 1) return 0;
    return reduce_orders_layout(nullptr, (size_t)E, (size_t)maxR, (size_t)n, nant, (size_t)K, nullptr);
}

extern "C" size_t frirl_hip_log_points_workspace_bytes(int32_t E, int32_t n_logs, int32_t T)
{
    if (E < 1 || n_logs < 1 || T < 1) return 0;
    return up16((size_t)E * (size_t)n_logs * (size_t)T);
}

template <int N>
static void launch_policy_map(const frirl_hip_rulebases *b, const frirl::MapArgs &m, int resident, double *qve, int32_t *best, double *actconc, hipStream_t s)
{
    const int amax = (long)m.n * m.A <= frirl::PM_BLOCK ? 1 : 4;       // one action per lane while an agent's (point, action) pairs fit one workgroup
    const frirl::MapShape shape = frirl::map_shape(m.A, amax);
    const int groups = (m.n + shape.ppp - 1) / shape.ppp;
    const int rcap = resident ? frirl::map_resident_rules(N, b->maxR) : 0;
    const size_t lds = (size_t)rcap * (N + 1) * sizeof(double);
    const dim3 grid((unsigned)b->E * (unsigned)groups), block(frirl::PM_BLOCK);
    if (amax == 1) hipLaunchKernelGGL((frirl::policy_map_kernel<N, 1>), grid, block, lds, s, b->rb, b->nrules, b->maxR, m, groups, rcap, qve, best, actconc);
    else hipLaunchKernelGGL((frirl::policy_map_kernel<N, 4>), grid, block, lds, s, b->rb, b->nrules, b->maxR, m, groups, rcap, qve, best, actconc);
}

extern "C" int frirl_hip_policy_map(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_map_points *pts,
                                    int32_t *best, double *actconc, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_policy_map";
    frirl::MapArgs m;
    int rc = check_map_args(who, t, b, agent, pts, &m);
    if (rc) return rc;
    if (!best) { set_error("%s: NULL best", who); return FRIRL_HIP_EINVAL; }
    if ((rc = check_workspace(who, workspace, workspace_bytes, frirl_hip_policy_map_workspace_bytes(t->nant, b->E, pts->n), "frirl_hip_policy_map_workspace_bytes")) ||
        (rc = check_device()))
        return rc;
    const int resident = opts().reduce_map_resident != 0;
    switch (t->nant) {
#define M(N) case N: launch_policy_map<N>(b, m, resident, static_cast<double *>(workspace), best, actconc, as_stream(stream)); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
    return check_launch(who);
}

extern "C" int frirl_hip_reduce_batch_map(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                          const frirl_hip_map_points *pts, int strategy, int32_t *kept, frirl_hip_reduce_map_result *results,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_reduce_batch_map";
    frirl::MapArgs m;
    int rc = check_map_args(who, t, b, agent, pts, &m);
    if (rc) return rc;
    if (!results) { set_error("%s: NULL results", who); return FRIRL_HIP_EINVAL; }
    if (strategy != 1 && strategy != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy); return FRIRL_HIP_EINVAL; }
    const size_t need = frirl_hip_reduce_batch_map_workspace_bytes(t->nant, b->E, b->maxR, pts->n);
    if ((rc = check_workspace(who, workspace, workspace_bytes, need, "frirl_hip_reduce_batch_map_workspace_bytes")) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    const size_t E = (size_t)b->E, M = (size_t)b->maxR;
    ReduceMapWs ws;
    reduce_map_layout(static_cast<char *>(workspace), E, M, (size_t)pts->n, t->nant, &ws);
    if ((rc = reduce_map_launch_order(who, *t, *b, pts->active, strategy, ws, s))) return rc;
    int32_t hdr[4];
    FRIRL_HIP_TRY(hipMemcpyAsync(hdr, ws.b.hdr, sizeof hdr, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    if ((rc = check_launch(who))) return rc;
    if (hdr[2]) { set_error("%s: agent %d: nrules outside 1..maxR=%d", who, hdr[2] - 1, b->maxR); return FRIRL_HIP_EINVAL; }
    reduce_map_launch_run(*t, *b, rant, m, opts().reduce_map_resident != 0, ws, s);
    FRIRL_HIP_TRY(hipMemcpyAsync(results, ws.res, sizeof(frirl_hip_reduce_map_result) * E, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    if (kept) FRIRL_HIP_TRY(hipMemcpyAsync(kept, ws.b.alive, sizeof(int32_t) * E * M, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    return check_launch(who);
}

extern "C" int frirl_hip_reduce_batch_map_orders(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                                 const frirl_hip_map_points *pts, int32_t K, const int32_t *orders, int32_t *kept,
                                                 frirl_hip_reduce_orders_result *results, int32_t *after_per_order, void *workspace, size_t workspace_bytes,
                                                 void *stream)
{
    static const char *who = "frirl_hip_reduce_batch_map_orders";
    frirl::MapArgs m;
    int rc = check_map_args(who, t, b, agent, pts, &m);
    if (rc) return rc;
    if (!results || !orders) { set_error("%s: NULL %s", who, results ? "orders" : "results"); return FRIRL_HIP_EINVAL; }
    if (K < 1 || K > FRIRL_HIP_REDUCE_MAX_ORDERS) { set_error("%s: K=%d orders outside 1..%d", who, K, FRIRL_HIP_REDUCE_MAX_ORDERS); return FRIRL_HIP_EINVAL; }
    if ((long long)b->E * K * pts->n > INT32_MAX) { set_error("%s: E=%d x K=%d x n=%d beyond 2^31 - 1", who, b->E, K, pts->n); return FRIRL_HIP_EINVAL; }
    const size_t need = frirl_hip_reduce_batch_map_orders_workspace_bytes(t->nant, b->E, b->maxR, pts->n, K);
    if ((rc = check_workspace(who, workspace, workspace_bytes, need, "frirl_hip_reduce_batch_map_orders_workspace_bytes")) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    const size_t E = (size_t)b->E, M = (size_t)b->maxR;
    ReduceOrdersWs ws;
    reduce_orders_layout(static_cast<char *>(workspace), E, M, (size_t)pts->n, t->nant, (size_t)K, &ws);
    if ((rc = reduce_orders_launch_check(who, *b, m, t->nant, orders, ws, s))) return rc;
    int32_t hdr[4];
    FRIRL_HIP_TRY(hipMemcpyAsync(hdr, ws.hdr, sizeof hdr, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    if ((rc = check_launch(who))) return rc;
    if (hdr[0]) { set_error("%s: agent %d: nrules outside 1..maxR=%d", who, INT32_MAX - hdr[0], b->maxR); return FRIRL_HIP_EINVAL; }
    if (hdr[1]) {
        const int ek = INT32_MAX - hdr[1];
        set_error("%s: agent %d, order k=%d: its first nrules entries are not a permutation of 0..nrules-1", who, ek / K, ek % K);
        return FRIRL_HIP_EINVAL;
    }
    reduce_orders_launch_run(*t, *b, rant, m, opts().reduce_map_resident != 0, orders, ws, s);
    FRIRL_HIP_TRY(hipMemcpyAsync(results, ws.res, sizeof(frirl_hip_reduce_orders_result) * E, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    if (kept) FRIRL_HIP_TRY(hipMemcpyAsync(kept, ws.alive, sizeof(int32_t) * E * M, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    if (after_per_order) FRIRL_HIP_TRY(hipMemcpyAsync(after_per_order, ws.after, sizeof(int32_t) * E * (size_t)K, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
    return check_launch(who);
}

extern "C" int frirl_hip_log_points(const frirl_hip_log_points_desc *lp, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_log_points";
    if (!lp || !lp->obs || !lp->q_obs || !lp->start || !lp->length || !lp->points || !lp->point_count || !lp->overflow ||
        (lp->only_successful && !lp->success)) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (lp->E < 1 || lp->n_logs < 1 || lp->T < 1 || lp->cap < 1 || lp->ns < 1 || lp->ns > 7) {
        set_error("%s: E=%d, n_logs=%d, T=%d, cap=%d must be >= 1 and ns=%d in 1..7", who, lp->E, lp->n_logs, lp->T, lp->cap, lp->ns);
        return FRIRL_HIP_EINVAL;
    }
    if ((long long)lp->E * lp->n_logs * lp->T > INT32_MAX || (long long)lp->E * lp->cap > INT32_MAX) {
        set_error("%s: E * n_logs * T or E * cap beyond 2^31 - 1", who);
        return FRIRL_HIP_EINVAL;
    }
    int rc = check_workspace(who, workspace, workspace_bytes, frirl_hip_log_points_workspace_bytes(lp->E, lp->n_logs, lp->T), "frirl_hip_log_points_workspace_bytes");
    if (rc || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    uint8_t *take = static_cast<uint8_t *>(workspace);
    hipLaunchKernelGGL(frirl::log_points_mark_kernel, dim3((unsigned)(lp->E * lp->n_logs)), dim3(frirl::LP_BLOCK), 0, s, *lp, take);
    switch (lp->ns) {
#define M(NS) case NS: hipLaunchKernelGGL(frirl::log_points_dedup_kernel<NS>, dim3((unsigned)lp->E), dim3(frirl::LP_BLOCK), 0, s, *lp, take); break;
        M(1) M(2) M(3) M(4) M(5) M(6) M(7)
#undef M
    }
    return check_launch(who);
}
