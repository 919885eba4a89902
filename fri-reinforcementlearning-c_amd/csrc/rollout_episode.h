// rollout_episode.h -- ONE greedy episode of frirl_test_run (src/frirl/frirl_test_run.c:66-70 -> frirl_episode.c:28-194 without the
// update at :155) by a group of G * H lanes against a read-only rule base.  Instantiated by rollout_shared_kernel (shared.hip), by the
// batched reduction's roll-out kernel (reduce_batch.hip), whose workgroups each point it at another agent's slab, and by the tiled form
// of the batched roll-out (rollout_batch.hip).  reduce_starts.hip keeps a copy of this loop with a per-row step cap: through a call it
// compiled to other code and ran 1 - 2 % slower (profiles/r24_rollout_loop.md, "tried and put aside").  The restartable form of the
// loop is rollout_record_episodes.h.
#pragma once
#include "shared_sweep.h"
#include "envs.h"

namespace frirl {

// Every lane of the workgroup must call it (shared_sweep's barriers), with the same rb / slot_g / R / max_steps; lanes with
// exists == false only help staging the tiles.  row = the row's id in the exploration stream; start = this row's start state
// ([NANT-1]) or NULL = ag.values_def.  grid_s: [NANT * FRIRL_HIP_MAX_GRID] doubles of LDS, filled here.
template <int NANT, int AMAX, int G, int H, bool EXCL, class POW>
__device__ __forceinline__ void rollout_episode(SharedTile<NANT> &tl, double *grid_s, const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                const double *__restrict__ rb, const uint8_t *__restrict__ slot_g, int R, int maxR,
                                                const frirl_hip_agent &ag, POW p, bool exists, uint32_t row, uint32_t mask,
                                                const double *__restrict__ start, int max_steps, int &steps, double &total, int &success,
                                                double (&states)[NANT - 1])
{
    constexpr int NS = NANT - 1;
    const GroupLane l = group_lane<G, H, AMAX>(ag.A);
    stage_agent<NANT>(tl, grid_s, ag);
    double cur[NS], qs[NS], q[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        states[k] = (exists && start) ? start[k] : ag.values_def[k];                                     // frirl_episode.c:46-48
        q[k] = observe_ve(u, ve, U, k, states[k]);
    }
    unsigned h0;
    int a;
    double bv;
    shared_sweep<NANT, AMAX, true, EXCL, G, H, POW>(tl, rb, slot_g, R, maxR, p, l.abeg, l.aend, l.nchunks, q, exists, mask, nullptr, h0, a, bv, l.h);   // :78 (un-quantised start state)
    group_first_max<G>(bv, a);
    a = e_greedy(ag, a, row, 0u, 0u);
    double action = grid_s[NS * FRIRL_HIP_MAX_GRID + a];                                                 // :82
    steps = 0;
    success = 0;
    total = 0.0;
    bool active = exists;
    for (int step = 1; step <= max_steps; step++) {                                                      // :86
        if (__syncthreads_count(active ? 1 : 0) == 0) break;                                             // every lane's episode has ended
        if (active) {
            double r;
            env_do_action(ag.env_kind, action, states, cur);                                             // :97
            env_get_reward(ag.env_kind, cur, r, success);                                                // :106
            total = total + r;                                                                           // :107
            env_quantize(ag.env_kind, NS, grid_s, ag.grid_len, ag.grid_div, cur, qs);                    // :112
#pragma unroll
            for (int k = 0; k < NS; k++) q[k] = observe_ve(u, ve, U, k, qs[k]);
        }
        int pa;
        shared_sweep<NANT, AMAX, true, EXCL, G, H, POW>(tl, rb, slot_g, R, maxR, p, l.abeg, l.aend, l.nchunks, q, active, mask, nullptr, h0, pa, bv, l.h);   // :148
        group_first_max<G>(bv, pa);
        if (active) {
            pa = e_greedy(ag, pa, row, 0u, (uint32_t)step);
            action = grid_s[NS * FRIRL_HIP_MAX_GRID + pa];                                               // :151
#pragma unroll
            for (int k = 0; k < NS; k++) states[k] = cur[k];                                             // :163-165
            steps++;                                                                                     // :174
            if (success == 1) active = false;                                                            // :183
        }
    }
}

}  // namespace frirl
