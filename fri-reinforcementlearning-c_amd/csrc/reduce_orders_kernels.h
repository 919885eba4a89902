// reduce_orders_kernels.h -- the map-validated try-remove reduction over SEVERAL candidate orders per agent
// (frirl_hip_reduce_batch_map_orders).  Included by reduce_run.hip ONLY, behind reduce_map_kernels.h: the trial loop is
// reduce_map_kernel's and the compaction is reduce_batch_compact.
//
// check   one workgroup per (agent, order): the rule count and the permutation test on the device; fills the order's PRIVATE slot bytes
//         (255 = present) through the test itself; the workgroup of order 0 also snaps the agent's points and resets `alive`
// trial   one workgroup per (agent, order): reduce_map_kernel's loop on the private slot bytes -- no rule base is written
// apply   one workgroup per agent: the order with the fewest survivors (ties: lowest k) is compacted into the rule base
#pragma once
#include "reduce_orders_ws.h"

namespace frirl {

// agents the reduction leaves alone (reduce_map_kernel's rule): inactive, a rule count outside 2..maxR, no point
__device__ __forceinline__ bool reduce_orders_untouched(const MapArgs &m, int e, int R, int maxR, bool &act, int &cnt)
{
    act = !m.active || m.active[e] != 0;
    cnt = m.point_count ? m.point_count[e] : m.n;
    cnt = cnt < 0 ? 0 : (cnt > m.n ? m.n : cnt);
    return !act || R < 2 || R > maxR || cnt == 0;
}

__global__ __launch_bounds__(256) void reduce_orders_check_kernel(const int32_t *__restrict__ nrules, int maxR, const MapArgs m, int ns,
                                                                  const int32_t *__restrict__ orders, ReduceOrdersWs w)
{
    __shared__ int bad;
    const int e = blockIdx.x / w.K, k = blockIdx.x - e * w.K, tid = threadIdx.x;
    const size_t M = (size_t)maxR;
    const int R = nrules[e];
    if (k == 0)
        for (int r = tid; r < maxR; r += 256) w.alive[(size_t)e * M + r] = r;
    bool act;
    int cnt;
    const bool untouched = reduce_orders_untouched(m, e, R, maxR, act, cnt);
    if (act && (R < 1 || R > maxR)) {                                  // uniform; reported by the host before anything is reduced
        if (k == 0 && tid == 0) atomicMax(&w.hdr[0], INT32_MAX - e);   // the lowest agent wins
        return;
    }
    if (untouched) return;                                             // uniform: its orders are not read
    if (k == 0) {
        double *qve = w.qve + (size_t)e * m.n * ns;
        const double *pts = m.points + (size_t)e * m.n * ns;
        for (int i = tid; i < cnt * ns; i += 256) qve[i] = observe_ve(m.u, m.ve, m.U, i % ns, pts[i]);
    }
    const size_t at = ((size_t)e * w.K + k) * M;
    uint8_t *slot = w.slot + at;
    const int32_t *ord = orders + at;
    if (tid == 0) bad = 0;
    for (int r = tid; r < R; r += 256) slot[r] = (uint8_t)0;
    __syncthreads();
    // R entries, each inside 0..R-1: a permutation iff every index is named at least once
    for (int j = tid; j < R; j += 256) {
        const int v = ord[j];
        if (v < 0 || v >= R) atomicOr(&bad, 1);
        else slot[v] = (uint8_t)255;
    }
    __syncthreads();
    for (int r = tid; r < R; r += 256)
        if (slot[r] != 255) atomicOr(&bad, 1);
    __syncthreads();
    if (tid == 0 && bad) atomicMax(&w.hdr[1], INT32_MAX - (e * w.K + k));
}

template <int NANT, int AMAX>
__global__ __launch_bounds__(PM_BLOCK) void reduce_orders_trial_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR, const MapArgs m,
                                                                        int rcap, const int32_t *__restrict__ orders, ReduceOrdersWs w)
{
    constexpr int NS = NANT - 1;
    extern __shared__ double lds_rules[];                              // [NANT + 1][rcap] columns, then [rcap] slot bytes
    __shared__ MapPassLds pl;
    __shared__ double ave[FRIRL_HIP_MAX_ACTIONS];
    const int e = blockIdx.x / w.K, k = blockIdx.x - e * w.K, tid = threadIdx.x;
    const size_t M = (size_t)maxR, ek = (size_t)e * w.K + k;
    const int R = nrules[e];
    bool act;
    int cnt;
    if (reduce_orders_untouched(m, e, R, maxR, act, cnt)) {            // uniform over the workgroup
        if (tid == 0) { w.after[ek] = R; w.tries[ek] = 0; }
        return;
    }
    const double *cols_g = rb + (size_t)e * (NANT + 1) * M;
    uint8_t *slot_g = w.slot + ek * M;                                 // all 255 below R: the check launch's permutation test
    const int32_t *order = orders + ek * M;
    const double *qve = w.qve + (size_t)e * m.n * NS;
    int32_t *best0 = w.best0 + ek * m.n;
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
    auto pass = [&](int cand, int pt0) {
        return resident ? map_pass<NANT, AMAX>(pl, lds_rules, (size_t)rcap, slot_l, R, cand, pw, ave, m.A, shape, qve, pt0, cnt, nullptr)
                        : map_pass<NANT, AMAX>(pl, cols_g, M, slot_g, R, cand, pw, ave, m.A, shape, qve, pt0, cnt, nullptr);
    };
    const int my_pt = tid / shape.chunks;
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
    if (tid == 0) { w.after[ek] = present; w.tries[ek] = tries; }
}

template <int NANT>
__global__ __launch_bounds__(256) void reduce_orders_apply_kernel(double *rb, int32_t *nrules, uint16_t *uidx, double *rant, int maxR, const MapArgs m,
                                                                  ReduceOrdersWs w)
{
    __shared__ int wave_kept[4];
    const int e = blockIdx.x, tid = threadIdx.x;
    const size_t M = (size_t)maxR;
    const int R = nrules[e];
    bool act;
    int cnt;
    if (reduce_orders_untouched(m, e, R, maxR, act, cnt)) {            // uniform over the workgroup
        if (tid == 0) { frirl_hip_reduce_orders_result r = {R, R, act ? cnt : 0, -1, 0, 0}; w.res[e] = r; }
        return;
    }
    int best = 0, left = w.after[(size_t)e * w.K];
    for (int k = 1; k < w.K; k++) {
        const int a = w.after[(size_t)e * w.K + k];
        if (a < left) { left = a; best = k; }                          // ties: the lowest k
    }
    const int tries = w.tries[(size_t)e * w.K + best];
    int Rn = R;
    if (left < R)
        Rn = reduce_batch_compact<NANT>(rb + (size_t)e * (NANT + 1) * M, rant ? rant + (size_t)e * NANT * M : nullptr,
                                        uidx ? uidx + (size_t)e * NANT * M : nullptr, w.alive + (size_t)e * M, w.slot + ((size_t)e * w.K + best) * M, M, R,
                                        1u, wave_kept);
    if (tid != 0) return;
    nrules[e] = Rn;
    frirl_hip_reduce_orders_result r = {R, Rn, cnt, best, tries, 0};
    w.res[e] = r;
}

}  // namespace frirl
