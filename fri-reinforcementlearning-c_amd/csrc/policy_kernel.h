// policy_kernel.h -- one greedy step of Q caller-stepped environments on ONE shared, read-only rule base: rollout_shared_kernel
// (shared.hip) cut at the step boundary, the way episode_kernel.h's EXT flag cut the fused learning step.  frirl_episode with
// reduction_state == 1 (reference src/frirl/frirl_episode.c:28-194 without the update at :155); do_action / get_reward /
// quantize_observations (:97,106,112) are the caller's and arrive as data (frirl_hip_agent_io), the per-row episode state
// lives in the caller's arrays (frirl_hip_policy_rows).  Instantiated per antecedent count in policy_i<N>.hip.
#pragma once
#include "shared_sweep.h"
#include "shape_ladder.h"
#include "envs.h"
#include <type_traits>

namespace frirl {

// begin != 0: rows with io.reset[q] != 0 (NULL: all) start an episode -- the greedy action of the UN-quantised observation (:46-48,78),
//             counters cleared; the other rows are not touched.
// begin == 0: rows with done[q] == 0 take the observation, reward and success flag of the last action and choose the next one (:148).
// G lanes split the actions and H lanes the rules of every conclusion of a row (shared_sweep); lane (h = 0, sub = 0) of a row
// writes.  The epsilon-greedy keys are rollout_shared_kernel's: (env_id_base + row, episode 0, step).
// PN: Shepard power = the default nant as a compile-time constant; else the agent's run-time power.
template <int NANT, int AMAX, int G, int H, bool EXCL, bool PN = true>
__global__ __launch_bounds__(SH_BLOCK) void policy_step_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                const frirl_hip_agent ag, const frirl_hip_policy_rows rows,
                                                                const frirl_hip_agent_io io, int begin)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    const int gl = threadIdx.x % GH, sub = gl % G, h = gl / G;      // group lane = (rule slice h, action slot sub)
    const int qi = blockIdx.x * EPB + threadIdx.x / GH;
    const bool exists = qi < rows.Q;
    const bool live = exists && (begin ? (!io.reset || io.reset[qi] != 0) : rows.done[qi] == 0);
    if (__syncthreads_count(live ? 1 : 0) == 0) return;             // every row of the workgroup is finished: nothing is staged
    using POW = typename std::conditional<PN, PowC<NANT>, PowU>::type;
    POW p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;
    const int apl = (ag.A + G - 1) / G;                              // actions per lane
    const int abeg = (sub * apl < ag.A) ? sub * apl : ag.A;
    const int aend = (abeg + apl < ag.A) ? abeg + apl : ag.A;
    const int nchunks = (apl + AMAX - 1) / AMAX;
    if ((int)threadIdx.x < ag.A) tl.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
    const uint32_t mask = (EXCL && exists) ? rows.exclude_mask[qi] : 0u;
    double q[NS];
    if (live) {
        double s[NS], qs[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) s[k] = io.obs[(size_t)qi * NS + k];
        if (begin) {
#pragma unroll
            for (int k = 0; k < NS; k++) qs[k] = s[k];                                                   // :78 (un-quantised start state)
        } else if (io.q_obs) {
#pragma unroll
            for (int k = 0; k < NS; k++) qs[k] = io.q_obs[(size_t)qi * NS + k];                          // the caller's quantize_observations
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
    const int R = nrules[0] < maxR ? nrules[0] : maxR;
    shared_sweep<NANT, AMAX, true, EXCL, G, H, POW>(tl, rb, rows.rule_slot, R, maxR, p, abeg, aend, nchunks, q, live, mask, nullptr, h0, a,
                                                    bv, h);                                              // :78 / :148
    group_first_max<G>(bv, a);
    if (!live || gl != 0) return;
    const int steps = begin ? 0 : rows.ep_steps[qi] + 1;                                                 // :174
    a = e_greedy(ag, a, (uint32_t)qi, 0u, (uint32_t)steps);
    io.action_out[qi] = ag.grid_values[NS * FRIRL_HIP_MAX_GRID + a];                                     // :82 / :151
    if (io.action_idx) io.action_idx[qi] = a;
    if (begin) {
        rows.ep_steps[qi] = 0;
        rows.ep_reward[qi] = 0.0;
        rows.success[qi] = 0;
        rows.done[qi] = 0;
    } else {
        const int success = io.success[qi];                                                              // :106
        rows.ep_steps[qi] = steps;
        rows.ep_reward[qi] = rows.ep_reward[qi] + io.reward[qi];                                         // :107
        rows.success[qi] = success;
        rows.done[qi] = (success == 1 || steps >= ag.max_steps) ? 1 : 0;                                 // :183, :86
    }
}

template <int N, int AMAX, int G, int H, bool PN = true>
static void launch_policy(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_policy_rows *rows,
                          const frirl_hip_agent_io *io, int begin, hipStream_t s)
{
    constexpr int EPB = SH_BLOCK / (G * H);
    const dim3 grid((rows->Q + EPB - 1) / EPB);
    if (rows->exclude_mask && rows->rule_slot)
        hipLaunchKernelGGL((policy_step_kernel<N, AMAX, G, H, true, PN>), grid, dim3(SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, *rows, *io, begin);
    else
        hipLaunchKernelGGL((policy_step_kernel<N, AMAX, G, H, false, PN>), grid, dim3(SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, *rows, *io, begin);
}

// G and H are chosen by policy.hip (lane_group / lane_slices); the compiled variant: for_shared_shape (shape_ladder.h)
template <int N>
static void launch_policy_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_policy_rows *rows,
                            const frirl_hip_agent_io *io, int begin, int G, int H, hipStream_t s)
{
    for_shared_shape<N>(ag, G, H, [&](auto sh) {
        using S = decltype(sh);
        launch_policy<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, rows, io, begin, s);
    });
}

}  // namespace frirl
