// rule_usage.hip -- which rules the greedy policy actually uses at a set of points (include/frirl_hip.h): batched
// FIVE_vag_concl_weight over every agent's points (frirl_hip_rule_usage) and the stable candidate order by a caller's keys
// (frirl_hip_rule_order).  The reduction that consumes the orders is frirl_hip_reduce_batch_map_orders (policy_map.hip).
#include "rule_usage.h"

namespace frirl {

// Launch 1, lane = (point, block of actions): policy_map_kernel's pass for the greedy action a*, then the lane that answers for the
// point walks the rules once more for a* alone: S (the bits of the map's weight sum) and the first exact hit.  All conditions in front
// of the barriers are uniform over the workgroup.
template <int NANT, int AMAX>
__global__ __launch_bounds__(PM_BLOCK) void rule_usage_points_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR, const MapArgs m,
                                                                      int groups, int rcap, const RuleUsageWs w, int32_t *__restrict__ best)
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
    const size_t at = (size_t)e * m.n + pt;
    if (first && pt >= cnt) {
        if (best) best[at] = -1;
        w.astar[at] = -1;
    }
    if (pt0 >= cnt) return;
    const size_t M = (size_t)maxR;
    const double *cols_g = rb + (size_t)e * (NANT + 1) * M;
    double *qve = w.qve + (size_t)e * m.n * NS;
    const double *pts = m.points + (size_t)e * m.n * NS;
    const int last = pt0 + shape.ppp < cnt ? pt0 + shape.ppp : cnt;
    for (int i = pt0 * NS + tid; i < last * NS; i += PM_BLOCK) qve[i] = observe_ve(m.u, m.ve, m.U, i % NS, pts[i]);
    if (tid < m.A) ave[tid] = m.action_ve[tid];
    const bool resident = R <= rcap;
    if (resident) map_stage<NANT>(lds_rules, rcap, cols_g, M, R);
    __syncthreads();
    const PowU pw{m.p};
    const int b = resident ? map_pass<NANT, AMAX>(pl, lds_rules, (size_t)rcap, nullptr, R, -1, pw, ave, m.A, shape, qve, pt0, cnt, nullptr)
                           : map_pass<NANT, AMAX>(pl, cols_g, M, nullptr, R, -1, pw, ave, m.A, shape, qve, pt0, cnt, nullptr);
    if (b < 0) return;                                                 // no barrier follows
    double q[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) q[k] = qve[(size_t)pt * NS + k];
    double S;
    unsigned h;
    if (resident) map_weight_sum<NANT>(lds_rules, (size_t)rcap, R, pw, q, ave[b], S, h);
    else map_weight_sum<NANT>(cols_g, M, R, pw, q, ave[b], S, h);
    if (best) best[at] = b;
    w.astar[at] = b;
    w.wsum[at] = S;
    w.hit[at] = h == FRIRL_HIP_NO_HIT ? -1 : (int)h;
}

// Launch 2, lane = rule: workgroup (e, block of RU_BLOCK rules).  A lane keeps its rule's columns in registers and walks the agent's
// points in list order from LDS tiles (every lane reads the same point: broadcast reads); one lane, plain adds in ascending j.
template <int NANT>
__global__ __launch_bounds__(RU_BLOCK) void rule_usage_sum_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR, const MapArgs m,
                                                                  int blocks, const RuleUsageWs w, double *__restrict__ sum, double *__restrict__ peak)
{
    constexpr int NS = NANT - 1;
    __shared__ double tq[RU_TILE][NS];
    __shared__ double tav[RU_TILE], tS[RU_TILE];
    __shared__ int th[RU_TILE];
    __shared__ double ave[FRIRL_HIP_MAX_ACTIONS];
    const int e = blockIdx.x / blocks, tid = threadIdx.x;
    const int r = (blockIdx.x - e * blocks) * RU_BLOCK + tid;
    const int R = nrules[e];
    if ((m.active && m.active[e] == 0) || R < 1 || R > maxR) return;   // uniform: the agent's rows are left untouched
    int cnt = m.point_count ? m.point_count[e] : m.n;
    cnt = cnt < 0 ? 0 : (cnt > m.n ? m.n : cnt);
    const size_t M = (size_t)maxR, row = (size_t)e * m.n;
    const bool mine = r < R;
    double c[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) c[k] = mine ? rb[((size_t)e * (NANT + 1) + k) * M + r] : 0.0;
    if (tid < m.A) ave[tid] = m.action_ve[tid];
    const PowU pw{m.p};
    double acc = 0.0, top = 0.0;
    for (int j0 = 0; j0 < cnt; j0 += RU_TILE) {
        const int nt = cnt - j0 < RU_TILE ? cnt - j0 : RU_TILE;
        __syncthreads();                                               // the last tile has been read; `ave` is visible
        for (int i = tid; i < nt * NS; i += RU_BLOCK) (&tq[0][0])[i] = w.qve[(row + j0) * NS + i];
        for (int i = tid; i < nt; i += RU_BLOCK) {
            const int a = w.astar[row + j0 + i];
            tav[i] = ave[a < 0 ? 0 : a];
            tS[i] = w.wsum[row + j0 + i];
            th[i] = w.hit[row + j0 + i];
        }
        __syncthreads();
        if (!mine) continue;                                           // the barriers are at the top of the loop
        for (int j = 0; j < nt; j++) {
            double wj;
            if (th[j] >= 0) {
                wj = th[j] == r ? 1.0 : 0.0;                           // FIVEVagConclWeight.c:92-98: the first hit takes all
            } else {
                const double d2 = map_rule_d2<NANT>(c, 1, 0, tq[j], tav[j]);
                wj = shepard_w(d2, pw) / tS[j];
            }
            acc = acc + wj;
            top = top < wj ? wj : top;
        }
    }
    if (r >= maxR) return;
    sum[(size_t)e * M + r] = mine ? acc : 0.0;
    if (peak) peak[(size_t)e * M + r] = mine ? top : 0.0;
}

constexpr int RO_TILE = 1024;            // keys staged in LDS per pass of the rank count

// q comes before r: by key, NaN keys after every number, equal keys (and NaNs among themselves) by index
__device__ __forceinline__ bool order_before(double kq, int q, double kr, int r, int descending)
{
    const bool nq = kq != kq, nr = kr != kr;
    if (nq || nr) return nq == nr ? q < r : nr;
    return (descending ? kq > kr : kq < kr) || (kq == kr && q < r);
}

// Order kernel: one workgroup per agent; the stable rank of every key by counting with the keys staged in LDS -- the ranking scheme of
// reduce_batch_order_kernel with the caller's keys (NULL: |Q|) and a place for NaNs.
__global__ __launch_bounds__(256) void rule_order_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int nant, int maxR,
                                                         const double *__restrict__ keys, int descending, const uint8_t *__restrict__ active,
                                                         int32_t *__restrict__ order)
{
    __shared__ double kq[RO_TILE];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int R = nrules[e];
    if ((active && active[e] == 0) || R < 1 || R > maxR) return;       // uniform over the workgroup: the row is left untouched
    const size_t row = (size_t)e * maxR;
    const double *col = keys ? keys + row : rb + ((size_t)e * (nant + 1) + nant) * maxR;
    auto key = [&](int i) { const double v = col[i]; return keys ? v : fabs(v); };
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        const double kr = r < R ? key(r) : 0.0;
        int rank = 0;
        for (int t0 = 0; t0 < R; t0 += RO_TILE) {
            const int n = R - t0 < RO_TILE ? R - t0 : RO_TILE;
            __syncthreads();
            for (int i = tid; i < n; i += 256) kq[i] = key(t0 + i);
            __syncthreads();
            if (r < R)
                for (int q = 0; q < n; q++) rank += order_before(kq[q], t0 + q, kr, r, descending) ? 1 : 0;
        }
        if (r < R) order[row + rank] = r;                              // a total order: the ranks are a permutation of 0..R-1
    }
}

}  // namespace frirl

extern "C" size_t frirl_hip_rule_usage_workspace_bytes(int32_t nant, int32_t E, int32_t n)
{
    if (nant < 2 || E < 1 || n < 1) return 0;
    return rule_usage_layout(nullptr, (size_t)E, (size_t)n, nant, nullptr);
}

template <int N>
static void launch_rule_usage(const frirl_hip_rulebases *b, const frirl::MapArgs &m, int resident, const frirl::RuleUsageWs &ws,
                              const frirl_hip_rule_usage_out *out, hipStream_t s)
{
    const int amax = (long)m.n * m.A <= frirl::PM_BLOCK ? 1 : 4;       // frirl_hip_policy_map's lane shape
    const frirl::MapShape shape = frirl::map_shape(m.A, amax);
    const int groups = (m.n + shape.ppp - 1) / shape.ppp;
    const int rcap = resident ? frirl::map_resident_rules(N, b->maxR) : 0;
    const size_t lds = (size_t)rcap * (N + 1) * sizeof(double);
    const dim3 grid((unsigned)b->E * (unsigned)groups), block(frirl::PM_BLOCK);
    if (amax == 1) hipLaunchKernelGGL((frirl::rule_usage_points_kernel<N, 1>), grid, block, lds, s, b->rb, b->nrules, b->maxR, m, groups, rcap, ws, out->best);
    else hipLaunchKernelGGL((frirl::rule_usage_points_kernel<N, 4>), grid, block, lds, s, b->rb, b->nrules, b->maxR, m, groups, rcap, ws, out->best);
    const int blocks = (b->maxR + frirl::RU_BLOCK - 1) / frirl::RU_BLOCK;
    hipLaunchKernelGGL(frirl::rule_usage_sum_kernel<N>, dim3((unsigned)b->E * (unsigned)blocks), dim3(frirl::RU_BLOCK), 0, s, b->rb, b->nrules, b->maxR, m,
                       blocks, ws, out->sum, out->peak);
}

extern "C" int frirl_hip_rule_usage(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_map_points *pts,
                                    const frirl_hip_rule_usage_out *out, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_rule_usage";
    frirl::MapArgs m;
    int rc = check_map_args(who, t, b, agent, pts, &m);
    if (rc) return rc;
    if (!out || !out->sum) { set_error("%s: NULL out / out->sum", who); return FRIRL_HIP_EINVAL; }
    if ((long long)b->E * ((b->maxR + frirl::RU_BLOCK - 1) / frirl::RU_BLOCK) > INT32_MAX) { set_error("%s: E=%d x maxR=%d: too many rule blocks", who, b->E, b->maxR); return FRIRL_HIP_EINVAL; }
    if ((rc = check_workspace(who, workspace, workspace_bytes, frirl_hip_rule_usage_workspace_bytes(t->nant, b->E, pts->n), "frirl_hip_rule_usage_workspace_bytes")) ||
        (rc = check_device()))
        return rc;
    frirl::RuleUsageWs ws;
    rule_usage_layout(static_cast<char *>(workspace), (size_t)b->E, (size_t)pts->n, t->nant, &ws);
    const int resident = opts().reduce_map_resident != 0;
    switch (t->nant) {
#define M(N) case N: launch_rule_usage<N>(b, m, resident, ws, out, as_stream(stream)); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
    return check_launch(who);
}

extern "C" int frirl_hip_rule_order(const frirl_hip_rulebases *b, int32_t nant, const double *keys, int descending, const uint8_t *active, int32_t *order,
                                    void *stream)
{
    static const char *who = "frirl_hip_rule_order";
    if (!b || !b->rb || !b->nrules || !order) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (b->E < 1 || b->maxR < 1) { set_error("%s: E=%d / maxR=%d < 1", who, b->E, b->maxR); return FRIRL_HIP_EINVAL; }
    if (nant < 2 || nant > 8) { set_error("%s: nant=%d outside 2..8", who, nant); return FRIRL_HIP_EINVAL; }
    if (descending != 0 && descending != 1) { set_error("%s: descending=%d (0 = ascending, 1 = descending)", who, descending); return FRIRL_HIP_EINVAL; }
    const int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL(frirl::rule_order_kernel, dim3((unsigned)b->E), dim3(256), 0, as_stream(stream), b->rb, b->nrules, nant, b->maxR, keys, descending, active,
                       order);
    return check_launch(who);
}
