// reduce_batch_kernels.h -- the protocol kernels of the batched reductions: order, open-round, close-round and result kernels and the
// in-place compaction, over the arrays of reduce_ws.h.  Included by reduce_run.hip ONLY: the library is built without relocatable
// device code, so a kernel is launched from the translation unit that defines it, and every launch of these sits behind ReduceRun
// (reduce_run.h).  Who runs the replays between open and close -- a roll-out kernel or the caller -- is not their business.
#pragma once
#include "reduce_ws.h"

namespace frirl {

constexpr int RB_ORDER_TILE = 1024;      // |Q| values staged in LDS per pass of the rank count

// Order kernel: one workgroup per agent.  Per-agent state, and the stable rank of every |Q| by counting (rw_before) with the
// consequents staged in LDS; workgroup 0 also builds the mask table.  Active agents join the first live list.
__global__ __launch_bounds__(256) void reduce_batch_order_kernel(const double *__restrict__ rb, const int32_t *__restrict__ nrules, int nant, int maxR,
                                                                 const uint8_t *__restrict__ active, int strategy, int max_steps, ReduceBatchWs ws)
{
    __shared__ double aq[RB_ORDER_TILE];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int R = nrules[e];
    const bool act = !active || active[e] != 0;
    const size_t row = (size_t)e * maxR;
    if (e == 0)
        for (int n = tid; n < ws.nodes; n += 256) ws.mask[n] = rw_node_mask((uint32_t)n);
    if (tid == 0) {
        ws.j[e] = 0; ws.d[e] = 0; ws.R0[e] = R; ws.rounds[e] = 0; ws.rollouts[e] = 0; ws.steps_inc[e] = 0; ws.cap[e] = max_steps;
        ws.prev[e] = 0.0;
    }
    for (int r = tid; r < maxR; r += 256) { ws.alive[row + r] = r; ws.slot[row + r] = (uint8_t)255; ws.order[row + r] = 0; }
    if (!act) return;                                                  // uniform over the workgroup
    if (R < 1 || R > maxR) {                                           // uniform; reported by the host before anything is reduced
        if (tid == 0) atomicCAS(&ws.hdr[2], 0, e + 1);
        return;
    }
    const double *qcol = rb + ((size_t)e * (nant + 1) + nant) * maxR;
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        const double ar = r < R ? fabs(qcol[r]) : 0.0;
        int rank = 0;
        for (int t0 = 0; t0 < R; t0 += RB_ORDER_TILE) {
            const int n = R - t0 < RB_ORDER_TILE ? R - t0 : RB_ORDER_TILE;
            __syncthreads();
            for (int i = tid; i < n; i += 256) aq[i] = fabs(qcol[t0 + i]);
            __syncthreads();
            if (r < R)
                for (int q = 0; q < n; q++) rank += rw_before(aq[q], t0 + q, ar, r, strategy) ? 1 : 0;
        }
        if (r < R) ws.order[row + rank] = r;                           // rank < R: at most R - 1 rules come before r
    }
    if (tid == 0) ws.live[0][atomicAdd(&ws.hdr[0], 1)] = e;
}

// Open-round kernel: one workgroup per live agent; d_e and the slot table of its next candidates.
__global__ __launch_bounds__(256) void reduce_batch_open_kernel(const int32_t *__restrict__ nrules, int maxR, int depth, int cur, ReduceBatchWs ws)
{
    __shared__ int cand[RW_MAX_DEPTH];
    const int e = ws.live[cur][blockIdx.x], tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) ws.hdr[cur ^ 1] = 0;             // the close kernel of this round appends to the other list
    const int j = ws.j[e], left = ws.R0[e] - j;
    const int d = left < depth ? left : depth;
    const int R = nrules[e];
    const size_t row = (size_t)e * maxR;
    if (tid < d) cand[tid] = ws.order[row + j + tid];
    if (tid == 0) ws.d[e] = d;
    __syncthreads();
    for (int r = tid; r < maxR; r += 256) {
        unsigned s = 255u;
        if (r < R) {
            const int a = ws.alive[row + r];
            for (int i = 0; i < d; i++) s = cand[i] == a ? (unsigned)i : s;
        }
        ws.slot[row + r] = (uint8_t)s;
    }
}

// In-place compaction of ONE agent's columns after a walk that ended with `bits` != 0 (both close kernels): chunks of 256 rules in
// index order, every chunk read into registers by all threads before any of it is written, and a write never lands above its read;
// then the vacated tail is zeroed.  Every thread of the 256-thread workgroup calls it with the same arguments; wave_kept: 4 ints of
// LDS.  Returns the number of rules left.
template <int NANT>
__device__ __forceinline__ int reduce_batch_compact(double *cols, double *ra, uint16_t *ui, int32_t *al, const uint8_t *sl, size_t M, int R, uint32_t bits, int *wave_kept)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        const bool keep = r < R && !rw_dropped(sl[r], bits);
        double v[NANT + 1], w[NANT];
        uint16_t x[NANT];
        int a = 0;
        if (keep) {
#pragma unroll
            for (int k = 0; k <= NANT; k++) v[k] = cols[k * M + r];
#pragma unroll
            for (int k = 0; k < NANT; k++) { w[k] = ra ? ra[k * M + r] : 0.0; x[k] = ui ? ui[k * M + r] : (uint16_t)0; }
            a = al[r];
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(bal);
        __syncthreads();                                           // the chunk is in registers; the wave counts are visible
        int pos = base + __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
        for (int i = 0; i < 4; i++) { pos += i < wave ? wave_kept[i] : 0; tot += wave_kept[i]; }
        if (keep && pos != r) {                                    // pos <= r
#pragma unroll
            for (int k = 0; k <= NANT; k++) cols[k * M + pos] = v[k];
#pragma unroll
            for (int k = 0; k < NANT; k++) { if (ra) ra[k * M + pos] = w[k]; if (ui) ui[k * M + pos] = x[k]; }
            al[pos] = a;
        }
        base += tot;
        __syncthreads();                                           // wave_kept is rewritten by the next chunk
    }
    for (int r = base + tid; r < R; r += 256) {                    // vacated tail: zero like five_remove_rule.c:64-80
#pragma unroll
        for (int k = 0; k <= NANT; k++) cols[k * M + r] = 0.0;
#pragma unroll
        for (int k = 0; k < NANT; k++) { if (ra) ra[k * M + r] = 0.0; if (ui) ui[k * M + r] = 0; }
    }
    return base;
}

// Close-round kernel: one workgroup per live agent.  first: the baseline replay sets steps_incremental, prev_reward and the
// agent's step cap.  Otherwise: walk the tree (every thread, same result), compact the rule base in place
// (reduce_batch_compact), advance the agent and append it to the next live list while candidates are left.
template <int NANT>
__global__ __launch_bounds__(256) void reduce_batch_close_kernel(double *__restrict__ rb, int32_t *__restrict__ nrules, uint16_t *__restrict__ uidx,
                                                                 double *__restrict__ rant, int maxR, int cur, int first, int max_steps,
                                                                 double good_above, double tol, ReduceBatchWs ws)
{
    __shared__ int wave_kept[4];
    const int e = ws.live[cur][blockIdx.x], tid = threadIdx.x;
    const size_t M = (size_t)maxR;
    const int R = nrules[e], d = first ? 0 : ws.d[e];
    const int steps_inc = first ? ws.steps[(size_t)e * ws.nodes] : ws.steps_inc[e];
    double prev = first ? ws.reward[(size_t)e * ws.nodes] : ws.prev[e];
    const uint32_t bits = rw_walk(d, ws.steps + (size_t)e * ws.nodes, ws.reward + (size_t)e * ws.nodes, steps_inc, prev, good_above, tol);
    int Rn = R;
    if (bits)                                                          // uniform: every thread walked the same tree
        Rn = reduce_batch_compact<NANT>(rb + (size_t)e * (NANT + 1) * M, rant ? rant + (size_t)e * NANT * M : nullptr,
                                        uidx ? uidx + (size_t)e * NANT * M : nullptr, ws.alive + (size_t)e * M, ws.slot + (size_t)e * M, M, R, bits,
                                        wave_kept);
    __syncthreads();                                                   // every thread has read the agent's state
    if (tid != 0) return;
    if (first) {
        ws.steps_inc[e] = steps_inc;
        ws.rollouts[e] = 1;
        ws.cap[e] = max_steps > steps_inc + 1 ? steps_inc + 1 : max_steps;     // a longer replay is rejected anyway (:212)
    } else {
        ws.rounds[e] += 1;
        ws.rollouts[e] += rw_nodes(d);
        nrules[e] = Rn;
    }
    ws.prev[e] = prev;
    const int j = ws.j[e] + d;
    ws.j[e] = j;
    if (j < ws.R0[e]) ws.live[cur ^ 1][atomicAdd(&ws.hdr[cur ^ 1], 1)] = e;
}

__global__ void reduce_batch_result_kernel(const int32_t *__restrict__ nrules, int E, ReduceBatchWs ws)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    frirl_hip_reduce_result r;
    r.rules_before = ws.R0[e];
    r.rules_after = nrules[e];
    r.rounds = ws.rounds[e];
    r.rollouts = ws.rollouts[e];
    r.steps_incremental = ws.steps_inc[e];
    r.reserved = 0;
    r.reward = ws.prev[e];
    ws.res[e] = r;
}

}  // namespace frirl
