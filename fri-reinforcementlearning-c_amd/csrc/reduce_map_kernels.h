// reduce_map_kernels.h -- the try-remove reduction validated on the policy map (frirl_hip_reduce_batch_map): ONE
// launch, one workgroup per agent, the loop over the candidates inside the kernel.  Included by reduce_run.hip ONLY, behind
// reduce_batch_kernels.h: the candidate order comes from reduce_batch_order_kernel and the compaction is reduce_batch_compact.
//
// Per agent: snap the points once; the map of the un-reduced rule base (best0); then for every candidate in order the map over the
// rules still present minus the candidate, pass by pass over the points, stopping at the first pass with a point whose greedy action
// differs.  An accepted removal only flips the rule's slot byte (255 -> 0); the columns are compacted once, at the end.
// resident: the agent's columns and slot bytes sit in LDS for the whole run; otherwise they are read from global memory (all lanes
// read the same rule at the same time: one broadcast line from the L1 per column).  Both run map_conclusions: the same bits.
#pragma once
#include "reduce_map_ws.h"

namespace frirl {

template <int NANT, int AMAX>
__global__ __launch_bounds__(PM_BLOCK) void reduce_map_kernel(double *rb, int32_t *nrules, uint16_t *uidx, double *rant, int maxR, const MapArgs m, int rcap,
                                                               ReduceMapWs w)
{
    constexpr int NS = NANT - 1;
    extern __shared__ double lds_rules[];                              // [NANT + 1][rcap] columns, then [rcap] slot bytes
    __shared__ MapPassLds pl;
    __shared__ double ave[FRIRL_HIP_MAX_ACTIONS];
    __shared__ int wave_kept[4];
    const int e = blockIdx.x, tid = threadIdx.x;
    const size_t M = (size_t)maxR;
    const int R = nrules[e];
    const bool act = !m.active || m.active[e] != 0;
    int cnt = m.point_count ? m.point_count[e] : m.n;
    cnt = cnt < 0 ? 0 : (cnt > m.n ? m.n : cnt);
    // untouched agents (uniform over the workgroup); an active agent with a bad rule count was refused by the host before this launch
    if (!act || R < 2 || R > maxR || cnt == 0) {
        if (tid == 0) { frirl_hip_reduce_map_result r = {R, R, act ? cnt : 0, 0}; w.res[e] = r; }
        return;
    }
    double *cols_g = rb + (size_t)e * (NANT + 1) * M;
    uint8_t *slot_g = w.b.slot + (size_t)e * M;
    const int32_t *order = w.b.order + (size_t)e * M;
    double *qve = w.qve + (size_t)e * m.n * NS;
    int32_t *best0 = w.best0 + (size_t)e * m.n;
    const double *pts = m.points + (size_t)e * m.n * NS;
    for (int i = tid; i < cnt * NS; i += PM_BLOCK) qve[i] = observe_ve(m.u, m.ve, m.U, i % NS, pts[i]);
    if (tid < m.A) ave[tid] = m.action_ve[tid];
    const bool resident = R <= rcap;
    uint8_t *slot_l = reinterpret_cast<uint8_t *>(lds_rules + (size_t)(NANT + 1) * rcap);
    if (resident) {
        map_stage<NANT>(lds_rules, rcap, cols_g, M, R);
        for (int r = tid; r < R; r += PM_BLOCK) slot_l[r] = (uint8_t)255;
    }
    __syncthreads();
    const MapShape shape = map_shape(m.A, AMAX);
    const PowU pw{m.p};
    // one pass in the agent's form; `cand` -1 = the map of the rules present
    auto pass = [&](int cand, int pt0) {
        return resident ? map_pass<NANT, AMAX>(pl, lds_rules, (size_t)rcap, slot_l, R, cand, pw, ave, m.A, shape, qve, pt0, cnt, nullptr)
                        : map_pass<NANT, AMAX>(pl, cols_g, M, slot_g, R, cand, pw, ave, m.A, shape, qve, pt0, cnt, nullptr);
    };
    const int my_pt = tid / shape.chunks;                              // the point whose answer map_pass hands this lane (block 0 lanes)
    for (int pt0 = 0; pt0 < cnt; pt0 += shape.ppp) {
        const int b = pass(-1, pt0);
        if (b >= 0) best0[pt0 + my_pt] = b;
    }
    __syncthreads();
    int present = R, tries = 0;
    for (int j = 0; j < R && present > 1; j++) {                       // the last remaining rule is never tried
        const int cand = order[j];
        int differs = 0;
        for (int pt0 = 0; pt0 < cnt && !differs; pt0 += shape.ppp) {
            const int b = pass(cand, pt0);
            differs = __syncthreads_or(b >= 0 && b != best0[pt0 + my_pt]);
        }
        tries += 1;
        if (differs) continue;
        if (tid == 0) {
            slot_g[cand] = (uint8_t)0;
            if (resident) slot_l[cand] = (uint8_t)0;
        }
        present -= 1;
        __syncthreads();
    }
    __syncthreads();
    int Rn = R;
    if (present < R)
        Rn = reduce_batch_compact<NANT>(cols_g, rant ? rant + (size_t)e * NANT * M : nullptr, uidx ? uidx + (size_t)e * NANT * M : nullptr,
                                        w.b.alive + (size_t)e * M, slot_g, M, R, 1u, wave_kept);
    if (tid != 0) return;
    nrules[e] = Rn;
    frirl_hip_reduce_map_result r = {R, Rn, cnt, tries};
    w.res[e] = r;
}

}  // namespace frirl
