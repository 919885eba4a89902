// policy_batch_kernel.h -- one greedy step of caller-stepped rows that belong to E DIFFERENT rule bases: policy_step_kernel
// (policy_kernel.h) with the agent taken from the workgroup index, the way reduce_batch_rollout_kernel (reduce_batch.hip) takes it.
// Row q = e * n + node is row `node` of agent e: it sweeps agent e's slab with agent e's slot table and step cap.  The step itself --
// observation handling, sweep, first maximum, epsilon-greedy, bookkeeping -- is policy_step_kernel's (frirl_episode.c:28-194 with
// reduction_state == 1).  Instantiated per antecedent count in policy_batch_i<N>.hip.
#pragma once
#include "policy_kernel.h"
#include "reduce_walk.h"

namespace frirl {

// what the kernel needs beyond the public row description: frirl_hip_policy_batch_begin / _observe fill it from the caller's struct,
// the batched reducer (policy_batch.hip) from its ReduceBatchWs
struct PolicyBatchArgs {
    frirl_hip_policy_batch_rows rows;
    const int32_t *list;          // [dev] agents served by the launch, one per `wpa` workgroups (rows.agents or a live list); NULL = 0..
    const int32_t *depth_of;      // [dev] [E] or NULL: agent e has the 2^depth_of[e] - 1 rows of its tree (instead of rows.row_count)
    int32_t E;                    // rule bases: entries of `list` outside 0..E-1 are skipped
    int32_t state_stride;         // ep_steps / ep_reward of row (e, node) sit at e * state_stride + node (the reducer: its tree size)
    int32_t mask_by_node;         // != 0: exclude_mask is indexed by node (one table for every agent) instead of by row
};

// begin / observe as policy_step_kernel.  `wpa` workgroups per served agent, each with 256 / (G * H) rows of that agent only, so
// everything in front of a barrier depends on the agent and on the workgroup's first row alone.  Rows node >= n_e do not exist:
// nothing of theirs is read or written.  After the step the rows of the workgroup that are not done are counted into
// *rows.rows_live: one integer atomic per workgroup.
//
// The try-remove rounds of the reducer against a set of start states (frirl_hip_batch_reducer_create_starts) pass ONE more kernel
// argument, a PolicyStartsArgs (ST...; without it the kernel and its arguments are what they were): an agent then has ns rows per
// node, row = node * ns + k being node `node` replayed from start k.  The mask is the node's (row / ns), the cap is start k's, and
// a row exists iff its node does (row < (2^d_e - 1) * ns) and start k is used; the holes in between are rows like those beyond n_e.
struct PolicyStartsArgs {
    const frirl_hip_reduce_start_result *res;      // [dev] [E][ns] res[e * ns + k].used != 0: start k of agent e is used
    const int32_t *cap;                            // [dev] [E][ns] step cap of the replays from start k
    int32_t ns;                                    // starts per agent
};
__device__ __forceinline__ const PolicyStartsArgs &only(const PolicyStartsArgs &st) { return st; }

template <int NANT, int AMAX, int G, int H, bool EXCL, bool PN = true, typename... ST>
__global__ __launch_bounds__(SH_BLOCK) void policy_batch_step_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                      const double *__restrict__ rb_all, const int32_t *__restrict__ nrules, int maxR,
                                                                      const frirl_hip_agent ag, const PolicyBatchArgs pa,
                                                                      const frirl_hip_agent_io io, int begin, int wpa, const ST... starts)
{
    constexpr bool STARTS = sizeof...(ST) == 1;
    static_assert(sizeof...(ST) == 0 || (STARTS && EXCL), "at most one extra argument, a PolicyStartsArgs, and only with exclusions");
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    const frirl_hip_policy_batch_rows &rows = pa.rows;
    const int slot_ix = blockIdx.x / wpa;
    const int e = pa.list ? pa.list[slot_ix] : slot_ix;
    if (e < 0 || e >= pa.E) return;                                  // uniform: not an agent of this batch
    const int row0 = (blockIdx.x % wpa) * EPB;
    const int n = rows.n;
    int ne = pa.depth_of ? rw_nodes(pa.depth_of[e]) : (rows.row_count ? rows.row_count[e] : n);
    if constexpr (STARTS) ne *= only(starts...).ns;
    ne = ne < 0 ? 0 : (ne > n ? n : ne);
    if (row0 >= ne) return;                                          // the whole workgroup, before the first barrier
    const int gl = threadIdx.x % GH, sub = gl % G, h = gl / G;      // group lane = (rule slice h, action slot sub)
    const int node = row0 + threadIdx.x / GH;
    bool exists = node < ne;
    int mask_ix = node;
    size_t start_ix = 0;                                             // STARTS: (agent, start) of the row
    if constexpr (STARTS) {
        const PolicyStartsArgs &st = only(starts...);
        mask_ix = node / st.ns;
        start_ix = (size_t)e * st.ns + (node - mask_ix * st.ns);
        exists = exists && st.res[start_ix].used != 0;
    }
    const size_t qi = (size_t)e * n + node, si = (size_t)e * pa.state_stride + node;
    const bool live = exists && (begin ? (!io.reset || io.reset[qi] != 0) : rows.done[qi] == 0);
    if (__syncthreads_count(live ? 1 : 0) == 0) {                    // no row of the workgroup takes this step: nothing is staged
        if (begin && io.reset && rows.rows_live) {                   // uniform; rows that were not restarted may still be running
            const int c = __syncthreads_count((exists && gl == 0 && rows.done[qi] == 0) ? 1 : 0);
            if (threadIdx.x == 0 && c) atomicAdd(rows.rows_live, c);
        }
        return;
    }
    using POW = typename std::conditional<PN, PowC<NANT>, PowU>::type;
    POW p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;
    const int apl = (ag.A + G - 1) / G;                              // actions per lane
    const int abeg = (sub * apl < ag.A) ? sub * apl : ag.A;
    const int aend = (abeg + apl < ag.A) ? abeg + apl : ag.A;
    const int nchunks = (apl + AMAX - 1) / AMAX;
    if ((int)threadIdx.x < ag.A) tl.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
    const uint32_t mask = (EXCL && exists) ? rows.exclude_mask[pa.mask_by_node ? (size_t)mask_ix : qi] : 0u;
    double q[NS];
    if (live) {
        double s[NS], qs[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) s[k] = io.obs[qi * NS + k];
        if (begin) {
#pragma unroll
            for (int k = 0; k < NS; k++) qs[k] = s[k];                                                   // :78 (un-quantised start state)
        } else if (io.q_obs) {
#pragma unroll
            for (int k = 0; k < NS; k++) qs[k] = io.q_obs[qi * NS + k];                                  // the caller's quantize_observations
        } else {
            env_quantize(FRIRL_HIP_ENV_EXTERNAL, NS, ag.grid_values, ag.grid_len, ag.grid_div, s, qs);   // :112, the generic rule
        }
#pragma unroll
        for (int k = 0; k < NS; k++) q[k] = observe_ve(u, ve, U, k, qs[k]);
    } else {
#pragma unroll
        for (int k = 0; k < NS; k++) q[k] = 0.0;
    }
    unsigned h0;
    int a;
    double bv;
    int R = nrules[e] < maxR ? nrules[e] : maxR;
    R = R < 0 ? 0 : R;
    const double *rb = rb_all + (size_t)e * (NANT + 1) * maxR;
    const uint8_t *slot_g = EXCL ? rows.rule_slot + (size_t)e * maxR : nullptr;
    shared_sweep<NANT, AMAX, true, EXCL, G, H, POW>(tl, rb, slot_g, R, maxR, p, abeg, aend, nchunks, q, live, mask, nullptr, h0, a, bv, h);   // :78 / :148
    group_first_max<G>(bv, a);
    int running = 0;                                                 // this lane's row is not done after the step
    if (exists && gl == 0) {
        if (!live) {
            running = (begin && rows.done[qi] == 0) ? 1 : 0;         // begin: a row that was not restarted
        } else {
            const int steps = begin ? 0 : rows.ep_steps[si] + 1;                                         // :174
            a = e_greedy(ag, a, (uint32_t)qi, 0u, (uint32_t)steps);
            io.action_out[qi] = ag.grid_values[NS * FRIRL_HIP_MAX_GRID + a];                             // :82 / :151
            if (io.action_idx) io.action_idx[qi] = a;
            if (begin) {
                rows.ep_steps[si] = 0;
                rows.ep_reward[si] = 0.0;
                rows.success[qi] = 0;
                rows.done[qi] = 0;
                running = 1;
            } else {
                int cap;
                if constexpr (STARTS) cap = only(starts...).cap[start_ix];
                else cap = rows.step_cap ? rows.step_cap[e] : ag.max_steps;
                const int success = io.success[qi];                                                      // :106
                const int done = (success == 1 || steps >= cap) ? 1 : 0;                                 // :183, :86
                rows.ep_steps[si] = steps;
                rows.ep_reward[si] = rows.ep_reward[si] + io.reward[qi];                                 // :107
                rows.success[qi] = success;
                rows.done[qi] = done;
                running = done ? 0 : 1;
            }
        }
    }
    if (!rows.rows_live) return;                                     // uniform
    const int c = __syncthreads_count(running);
    if (threadIdx.x == 0 && c) atomicAdd(rows.rows_live, c);
}

template <int N, int AMAX, int G, int H, bool PN = true>
static void launch_policy_batch(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const PolicyBatchArgs *pa,
                                const frirl_hip_agent_io *io, int begin, int nlist, const PolicyStartsArgs *st, hipStream_t s)
{
    constexpr int EPB = SH_BLOCK / (G * H);
    const int wpa = (pa->rows.n + EPB - 1) / EPB;
    const dim3 grid((unsigned)nlist * wpa);
    if (st)
        hipLaunchKernelGGL((policy_batch_step_kernel<N, AMAX, G, H, true, PN, PolicyStartsArgs>), grid, dim3(SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, *pa, *io, begin, wpa, *st);
    else if (pa->rows.exclude_mask && pa->rows.rule_slot)
        hipLaunchKernelGGL((policy_batch_step_kernel<N, AMAX, G, H, true, PN>), grid, dim3(SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, *pa, *io, begin, wpa);
    else
        hipLaunchKernelGGL((policy_batch_step_kernel<N, AMAX, G, H, false, PN>), grid, dim3(SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, *pa, *io, begin, wpa);
}

// the lane shapes of the batched reduction's roll-out kernel (for_batch_shape, shape_ladder.h); H is chosen by policy_batch.hip
template <int N>
static void launch_policy_batch_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const PolicyBatchArgs *pa,
                                  const frirl_hip_agent_io *io, int begin, int nlist, int H, const PolicyStartsArgs *st, hipStream_t s)
{
    for_batch_shape<N>(ag, H, [&](auto sh) {
        using S = decltype(sh);
        launch_policy_batch<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, pa, io, begin, nlist, st, s);
    });
}

}  // namespace frirl
