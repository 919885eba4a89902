// rollout_record_episodes.h -- K greedy episodes of frirl_test_run (rollout_episode.h: frirl_episode.c:28-194 without the update at :155)
// by a group of G * H lanes against a read-only rule base, EVERY step written as a record of a demonstration log (struct
// frirl_hip_demonstration, include/frirl_hip.h): the body of rollout_record_kernel (rollout_record.hip).
//
// One step loop for the whole workgroup.  A group whose episode ended begins its next one in the following iteration (its sweep then
// takes the un-quantised start state, :78), so a group with short episodes does not idle while a neighbour runs to max_steps; the loop
// ends when every group has finished all its episodes or filled its log.
#pragma once
#include "shared_sweep.h"
#include "envs.h"

namespace frirl {

// Every lane of the workgroup must call it (shared_sweep's barriers), with the same rb / R; lanes with exists == false only help
// staging the tiles.  q = the log's index (its id in the exploration stream; episode k draws from (env_id_base + q, k, step)).
// grid_s: [NANT * FRIRL_HIP_MAX_GRID] doubles of LDS, filled here.
template <int NANT, int AMAX, int G, int H, class POW>
__device__ __forceinline__ void rollout_record_episodes(SharedTile<NANT> &tl, double *grid_s, const double *__restrict__ u, const double *__restrict__ ve,
                                                        int U, const double *__restrict__ rb, int R, int maxR, const frirl_hip_agent &ag, POW p,
                                                        bool exists, size_t q, const frirl_hip_rollout_log &lg)
{
    constexpr int NS = NANT - 1;
    const GroupLane l = group_lane<G, H, AMAX>(ag.A);
    const bool leader = l.leader;
    stage_agent<NANT>(tl, grid_s, ag);
    const int K = lg.episodes, T = lg.T;
    const size_t rec0 = q * (size_t)T, ep0 = q * (size_t)K;         // first record / first episode of this log
    double states[NS], cur[NS], qs[NS], qv[NS], total = 0.0, action = 0.0;
#pragma unroll
    for (int k = 0; k < NS; k++) { states[k] = 0.0; cur[k] = 0.0; qs[k] = 0.0; qv[k] = 0.0; }
    int ep = 0, pos = 0, steps = 0, success = 0;
    bool fresh = true, fin = !exists;                                // T >= 2: episode 0 always begins
    for (;;) {
        if (__syncthreads_count(fin ? 0 : 1) == 0) break;            // every log of the workgroup is complete
        double r = 0.0;
        if (!fin) {
            if (fresh) {
                const double *start = lg.start_states ? lg.start_states + (ep0 + (size_t)ep) * NS : nullptr;
#pragma unroll
                for (int k = 0; k < NS; k++) {
                    states[k] = start ? start[k] : ag.values_def[k];                                     // frirl_episode.c:46-48
                    qv[k] = observe_ve(u, ve, U, k, states[k]);
                }
                steps = 0;
                success = 0;
                total = 0.0;
            } else {
                env_do_action(ag.env_kind, action, states, cur);                                         // :97
                env_get_reward(ag.env_kind, cur, r, success);                                            // :106
                total = total + r;                                                                       // :107
                env_quantize(ag.env_kind, NS, grid_s, ag.grid_len, ag.grid_div, cur, qs);                // :112
#pragma unroll
                for (int k = 0; k < NS; k++) qv[k] = observe_ve(u, ve, U, k, qs[k]);
            }
        }
        unsigned h0;
        int pa;
        double bv;
        shared_sweep<NANT, AMAX, true, false, G, H, POW>(tl, rb, nullptr, R, maxR, p, l.abeg, l.aend, l.nchunks, qv, !fin, 0u, nullptr, h0, pa, bv, l.h);   // :78 / :148
        group_first_max<G>(bv, pa);
        if (!fin) {
            const size_t rec = rec0 + (size_t)pos;                   // pos < T: a log with fewer than 2 free records begins no episode, a full one is finished
            bool ended;
            if (fresh) {
                pa = e_greedy(ag, pa, (uint32_t)q, (uint32_t)ep, 0u);
                if (leader) {
#pragma unroll
                    for (int k = 0; k < NS; k++) {
                        lg.obs[rec * NS + k] = states[k];
                        if (lg.q_obs) lg.q_obs[rec * NS + k] = 0.0;
                    }
                    lg.reward[rec] = 0.0;
                    lg.success[rec] = 0;
                    lg.start[rec] = 1;
                    lg.action[rec] = pa;
                }
                fresh = false;
                ended = ag.max_steps < 1;                                                                // :86
            } else {
                steps++;                                                                                 // :174
                pa = e_greedy(ag, pa, (uint32_t)q, (uint32_t)ep, (uint32_t)steps);
#pragma unroll
                for (int k = 0; k < NS; k++) states[k] = cur[k];                                         // :163-165
                if (leader) {
#pragma unroll
                    for (int k = 0; k < NS; k++) {
                        lg.obs[rec * NS + k] = cur[k];
                        if (lg.q_obs) lg.q_obs[rec * NS + k] = qs[k];
                    }
                    lg.reward[rec] = r;
                    lg.success[rec] = success;
                    lg.start[rec] = 0;
                    lg.action[rec] = pa;                             // the terminal record carries its pick too (:148)
                }
                ended = success == 1 || steps >= ag.max_steps;                                           // :183, :86
            }
            action = grid_s[NS * FRIRL_HIP_MAX_GRID + pa];                                               // :82 / :151
            pos++;
            if (ended || pos >= T) {                                 // the episode is over, or cut where the log is full
                if (leader) {
                    if (lg.ep_steps) lg.ep_steps[ep0 + ep] = steps;
                    if (lg.ep_reward) lg.ep_reward[ep0 + ep] = total;
                    if (lg.ep_success) lg.ep_success[ep0 + ep] = success;
                }
                ep++;
                fresh = true;
                if (ep >= K || T - pos < 2) {                        // a lone start record teaches nothing: the episode is not begun
                    fin = true;
                    if (leader) {
                        for (int k = ep; k < K; k++) {
                            if (lg.ep_steps) lg.ep_steps[ep0 + k] = -1;
                            if (lg.ep_reward) lg.ep_reward[ep0 + k] = 0.0;
                            if (lg.ep_success) lg.ep_success[ep0 + k] = 0;
                        }
                        lg.length[q] = pos;
                    }
                }
            }
        }
    }
}

}  // namespace frirl
