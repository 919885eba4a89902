// shape_ladder.h -- host side: from the run-time shape of a roll-out (actions, Shepard power, lanes per row G, rule slices H) to the
// compiled variant <AMAX, G, H, PN> of its kernel.  One ladder per family of kernels, each calling f(LaneShape<...>{}) once:
//   for_shared_shape   ONE shared rule base: rollout_shared_kernel (shared.hip) and policy_step_kernel (policy_kernel.h)
//   for_batch_shape    every agent's own rule base: reduce_batch_rollout_kernel (reduce_batch.hip) and policy_batch_step_kernel
// The two stay apart: together they would instantiate H = 16 and G = 1 variants that nobody launches.
#pragma once
#include "device_common.h"

namespace frirl {

// AMAX conclusions per lane and pass, G lanes per row, H rule slices per conclusion; PN: the Shepard power is the default nant
template <int AMAX_, int G_, int H_, bool PN_>
struct LaneShape {
    static constexpr int AMAX = AMAX_, G = G_, H = H_;
    static constexpr bool PN = PN_;
};

// H = 1 / 4 / 8; a run-time Shepard power and G = 1 are instantiated without rule slices
template <int AMAX, int G, bool PN, class F>
static void for_slices(int H, F &&f)
{
    if constexpr (PN && G > 1) {
        if (H == 8) return f(LaneShape<AMAX, G, 8, PN>{});
        if (H == 4) return f(LaneShape<AMAX, G, 4, PN>{});
    }
    f(LaneShape<AMAX, G, 1, PN>{});
}

template <bool PN, class F>
static void for_shared_group(int A, int G, int H, F &&f)
{
    if (G == 4) for_slices<1, 4, PN>(H, f);           // one conclusion per lane, A <= 4
    else if (G == 8) for_slices<4, 8, PN>(H, f);      // chunks of 4
    else if (A <= 4) for_slices<4, 1, PN>(H, f);
    else for_slices<8, 1, PN>(H, f);
}

// G = 1, 4 (A <= 4) or 8 (A > 4), H = 1 / 4 / 8: lane_group / lane_slices below
template <int N, class F>
static void for_shared_shape(const frirl_hip_agent *ag, int G, int H, F &&f)
{
    if (ag->p > 0 && ag->p != N) for_shared_group<false>(ag->A, G, H, f);
    else for_shared_group<true>(ag->A, G, H, f);
}

// G = 4 lanes per row with one conclusion each for up to 4 actions, else 8 lanes with chunks of 4; H = 1 / 4 / 8 rule slices,
// 16 (G = 4) = a full wave per row
template <int N, class F>
static void for_batch_shape(const frirl_hip_agent *ag, int H, F &&f)
{
    const bool few = ag->A <= 4;
    if (ag->p > 0 && ag->p != N) return few ? for_slices<1, 4, false>(H, f) : for_slices<4, 8, false>(H, f);
    if (few && H == 16) return f(LaneShape<1, 4, 16, true>{});
    return few ? for_slices<1, 4, true>(H, f) : for_slices<4, 8, true>(H, f);
}

}  // namespace frirl

namespace frirl_host {

// Lanes per row of a shared-base roll-out with Q rows: 1 once the rows alone fill the chip, else the actions split over 4 (A <= 4)
// or 8 lanes.  `forced`: the option rollout_group / policy_group, 0 = by shape.
static int lane_group(int forced, int Q, int A)
{
    if (forced == 1 || (forced == 4 && A <= 4) || (forced == 8 && A > 4)) return forced;
    if (A < 2 || Q >= 131072) return 1;
    return A <= 4 ? 4 : 8;
}

// Rule slices per conclusion (G > 1 only): the replays of the reduction run ~1000 rows, one step is then a latency chain over the
// rules -- 4 or 8 lanes share it while the launch stays under ~2048 waves.  `forced`: the option rollout_slices / policy_slices.
static int lane_slices(int forced, int Q, int G)
{
    if (G == 1) return 1;
    if (forced == 1 || forced == 4 || forced == 8) return forced;
    const long waves1 = ((long)Q * G + 63) / 64;
    return waves1 * 8 <= 2048 ? 8 : (waves1 * 4 <= 2048 ? 4 : 1);
}

}  // namespace frirl_host
