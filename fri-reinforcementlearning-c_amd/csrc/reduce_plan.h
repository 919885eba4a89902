// reduce_plan.h -- host side of the speculative try-remove reduction (frirl_sequential_run.c:170-350; include/frirl_hip.h):
// the host copies of the rule base, the slot and mask tables of a round's accept/reject tree and the compaction; the order, the
// masks, the walk and the drop flags themselves are reduce_walk.h's, as in the batched reduction's kernels.  One helper for both forms:
// frirl_hip_reduce_shared (shared.hip: the replays run the demo dynamics in the kernel) and frirl_hip_reducer_* (policy.hip: the
// caller steps the environment).  Neither form owns a second copy of this logic.
#pragma once
#include "device_common.h"
#include "reduce_walk.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace frirl_host {

struct ReducePlan {
    const char *who = "";
    int nant = 0, maxR = 0, depth = 0;
    frirl_hip_rulebases b = {};
    double *rant = nullptr;                   // [dev] raw antecedents compacted alongside, or NULL
    std::vector<double> slab, rants;          // host copies of the rule base (and rant), compacted round by round
    std::vector<uint16_t> idx;
    std::vector<int> order;                   // candidates in trial order (original rule indices)
    std::vector<int> alive;                   // original index of the rule in each current slot
    std::vector<int> where;                   // current slot of each original rule, -1 = removed
    std::vector<uint8_t> slot;                // [maxR] candidate slot of every current rule, 255 = none (this round)
    std::vector<uint32_t> mask;               // [lanes_max] exclude mask of every tree node (this round)
    int R0 = 0, R = 0, j = 0, d = 0, rounds = 0, rollouts = 0, steps_inc = 0;
    double prev_reward = 0.0;

    int lanes_max() const { return frirl::rw_nodes(depth); }
    bool finished() const { return j >= R0; }

    // host copies of the rule base and the candidate order; synchronises `s`
    int load(const char *who_, const frirl_hip_tables *t, const frirl_hip_rulebases *b_, double *rant_, int strategy, int depth_, hipStream_t s)
    {
        who = who_; nant = t->nant; maxR = b_->maxR; depth = depth_; b = *b_; rant = rant_;
        const size_t col = (size_t)maxR;
        int32_t r0 = 0;
        FRIRL_HIP_TRY(hipMemcpyAsync(&r0, b.nrules, sizeof r0, hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
        FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
        if (r0 < 1 || r0 > maxR) { set_error("%s: nrules=%d outside 1..maxR=%d", who, r0, maxR); return FRIRL_HIP_EINVAL; }
        R0 = R = r0;
        slab.resize((size_t)(nant + 1) * col);
        FRIRL_HIP_TRY(hipMemcpyAsync(slab.data(), b.rb, slab.size() * sizeof(double), hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH);
        if (rant) { rants.resize((size_t)nant * col); FRIRL_HIP_TRY(hipMemcpyAsync(rants.data(), rant, rants.size() * sizeof(double), hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH); }
        if (b.uidx) { idx.resize((size_t)nant * col); FRIRL_HIP_TRY(hipMemcpyAsync(idx.data(), b.uidx, idx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, s), who, return FRIRL_HIP_ELAUNCH); }
        FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
        // candidate order: the reference rescans for the first minimum (strategy 1) or the first maximum (strategy 2) of the
        // not-yet-tested consequents after every episode; the consequents never change and removals keep the relative rule order,
        // so that is the strict total order rw_before, fixed up front
        const double *qcol = slab.data() + (size_t)nant * col;
        order.resize(R0);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](int a, int c) { return frirl::rw_before(std::fabs(qcol[a]), a, std::fabs(qcol[c]), c, strategy); });
        alive.resize(R0);
        std::iota(alive.begin(), alive.end(), 0);
        where.resize(R0);
        slot.resize(col);
        mask.resize(lanes_max());
        for (size_t n = 0; n < mask.size(); n++) mask[n] = frirl::rw_node_mask((uint32_t)n);     // the same in every round
        j = d = rounds = 0;
        return FRIRL_HIP_OK;
    }

    // baseline replay on the un-reduced rule base (:196-198 and the first loop iteration, :204-206)
    void set_baseline(int steps, double reward) { steps_inc = steps; prev_reward = reward; rollouts = 1; }

    // replays of a round are capped at steps_incremental + 1 steps (a longer episode is rejected anyway, :212)
    int capped_steps(int max_steps) const { return max_steps > steps_inc + 1 ? steps_inc + 1 : max_steps; }

    // slots and masks of the next round's tree, uploaded to d_slot [maxR] / d_mask [lanes]; returns its lanes (0: finished) in *lanes
    int open_round(void *d_slot, void *d_mask, hipStream_t s, int *lanes)
    {
        *lanes = 0;
        if (finished()) return FRIRL_HIP_OK;
        d = std::min(depth, R0 - j);
        const int n = frirl::rw_nodes(d);
        std::fill(where.begin(), where.end(), -1);
        for (int i = 0; i < R; i++) where[alive[i]] = i;
        std::fill(slot.begin(), slot.end(), (uint8_t)255);
        for (int i = 0; i < d; i++) slot[where[order[j + i]]] = (uint8_t)i;
        FRIRL_HIP_TRY(hipMemcpyAsync(d_slot, slot.data(), (size_t)maxR, hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
        FRIRL_HIP_TRY(hipMemcpyAsync(d_mask, mask.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
        *lanes = n;
        return FRIRL_HIP_OK;
    }

    // walk the tree along the outcomes that happened (steps / reward: host, one entry per node), compact the rule base; synchronises `s`
    int close_round(const int32_t *steps, const double *reward, double reward_good_above, double reward_tolerance, hipStream_t s)
    {
        const size_t col = (size_t)maxR;
        rounds++;
        rollouts += frirl::rw_nodes(d);
        const uint32_t bits = frirl::rw_walk(d, steps, reward, steps_inc, prev_reward, reward_good_above, reward_tolerance);   // :212, :222
        if (bits) {                                                   // five_remove_rule of every accepted candidate: compact all columns
            int w = 0;
            for (int r = 0; r < R; r++) {
                if (frirl::rw_dropped(slot[r], bits)) continue;
                if (w != r) {
                    for (int k = 0; k <= nant; k++) slab[(size_t)k * col + w] = slab[(size_t)k * col + r];
                    if (rant) for (int k = 0; k < nant; k++) rants[(size_t)k * col + w] = rants[(size_t)k * col + r];
                    if (b.uidx) for (int k = 0; k < nant; k++) idx[(size_t)k * col + w] = idx[(size_t)k * col + r];
                    alive[w] = alive[r];
                }
                w++;
            }
            for (int r = w; r < R; r++) {                             // vacated tail: zero like the reference's memset (five_remove_rule.c:64-80)
                for (int k = 0; k <= nant; k++) slab[(size_t)k * col + r] = 0.0;
                if (rant) for (int k = 0; k < nant; k++) rants[(size_t)k * col + r] = 0.0;
                if (b.uidx) for (int k = 0; k < nant; k++) idx[(size_t)k * col + r] = 0;
            }
            R = w;
            alive.resize(R);
            const int32_t Rn = R;
            FRIRL_HIP_TRY(hipMemcpyAsync(b.rb, slab.data(), slab.size() * sizeof(double), hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
            if (rant) FRIRL_HIP_TRY(hipMemcpyAsync(rant, rants.data(), rants.size() * sizeof(double), hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
            if (b.uidx) FRIRL_HIP_TRY(hipMemcpyAsync(b.uidx, idx.data(), idx.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
            FRIRL_HIP_TRY(hipMemcpyAsync(b.nrules, &Rn, sizeof Rn, hipMemcpyHostToDevice, s), who, return FRIRL_HIP_ELAUNCH);
            FRIRL_HIP_TRY(hipStreamSynchronize(s), who, return FRIRL_HIP_ELAUNCH);
        }
        j += d;
        return FRIRL_HIP_OK;
    }

    void result(int32_t *kept, frirl_hip_reduce_result *res) const
    {
        if (kept) for (int i = 0; i < R; i++) kept[i] = alive[i];
        if (!res) return;
        res->rules_before = R0;
        res->rules_after = R;
        res->rounds = rounds;
        res->rollouts = rollouts;
        res->steps_incremental = steps_inc;
        res->reserved = 0;
        res->reward = prev_reward;
    }
};

}  // namespace frirl_host
