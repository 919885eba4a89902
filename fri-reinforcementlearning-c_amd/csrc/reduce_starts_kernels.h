// reduce_starts_kernels.h -- the protocol kernels of a reduction against a set of start states, next to those of
// reduce_batch_kernels.h: init, close-round and result kernel over the per-start arrays (ReduceStartsWs, reduce_ws.h).  Included by
// reduce_run.hip only, like reduce_batch_kernels.h.  The close kernel's STEPPED flag selects the row layout its walk reads: compact
// (row = node * K_e + ki, the in-kernel roll-outs of reduce_starts.hip) or fixed (row = node * n + k, the caller-stepped reducer).
#pragma once
#include "reduce_batch_kernels.h"

namespace frirl {

// Init kernel: one workgroup per agent; the per-start state of an agent that never takes part stays as written here.
__global__ __launch_bounds__(256) void reduce_starts_init_kernel(const int32_t *__restrict__ start_count, ReduceStartsWs ws)
{
    const int e = blockIdx.x, tid = threadIdx.x, n = ws.n;
    if (tid == 0) {
        int c = start_count ? start_count[e] : n;
        ws.cnt[e] = c < 1 ? 1 : (c > n ? n : c);
        ws.K[e] = 0;
        ws.capmax[e] = 0;
    }
    for (int k = tid; k < n; k += 256) {
        const size_t i = (size_t)e * n + k;
        ws.used[i] = 0; ws.steps_inc[i] = -1; ws.cap[i] = 0; ws.prev[i] = 0.0;
        ws.res[i].used = 0; ws.res[i].steps_incremental = -1; ws.res[i].baseline_reward = 0.0; ws.res[i].reward = 0.0;
    }
}

// Close-round kernel: one workgroup per live agent.  first: thread 0 takes every participating start's baseline (steps_inc, prev,
// cap), decides which starts are used and lists them; an agent with no used start is not appended to the live list.  Otherwise:
// thread 0 walks the tree over nodes x starts (it alone reads and writes the agent's prev array), the workgroup compacts.
// STEPPED: the replays of a node sit at node * n + k for start k (the caller-stepped rows) instead of node * K_e + ki; the baseline
// replays sit at k in both forms.
template <int NANT, bool STEPPED = false>
__global__ __launch_bounds__(256) void reduce_starts_close_kernel(double *__restrict__ rb, int32_t *__restrict__ nrules, uint16_t *__restrict__ uidx,
                                                                  double *__restrict__ rant, int maxR, int cur, int first, int max_steps,
                                                                  double good_above, double tol, int drop_bad, ReduceStartsWs ws)
{
    __shared__ int wave_kept[4];
    __shared__ uint32_t bits_s;
    const int e = ws.b.live[cur][blockIdx.x], tid = threadIdx.x, n = ws.n;
    const size_t M = (size_t)maxR, en = (size_t)e * n, rows0 = (size_t)e * ws.b.nodes * n;
    if (first) {                                                       // uniform
        if (tid != 0) return;
        const int cnt = ws.cnt[e];
        int K = 0, capmax = 0;
        for (int k = 0; k < cnt; k++) {
            const int st = ws.b.steps[rows0 + k];
            const double rw = ws.b.reward[rows0 + k];
            const int cap = max_steps > st + 1 ? st + 1 : max_steps;   // a longer replay is rejected anyway (:212)
            const bool use = !drop_bad || rw > good_above;
            ws.steps_inc[en + k] = st;
            ws.prev[en + k] = rw;
            ws.cap[en + k] = cap;
            ws.res[en + k].used = use ? 1 : 0;
            ws.res[en + k].steps_incremental = st;
            ws.res[en + k].baseline_reward = rw;
            if (use) {
                ws.used[en + K++] = k;
                capmax = cap > capmax ? cap : capmax;
            }
        }
        const int k0 = K ? ws.used[en] : 0;
        ws.K[e] = K;
        ws.capmax[e] = capmax;
        ws.b.steps_inc[e] = ws.steps_inc[en + k0];
        ws.b.prev[e] = ws.prev[en + k0];
        ws.b.rollouts[e] = cnt;
        if (K > 0 && ws.b.R0[e] > 0) ws.b.live[cur ^ 1][atomicAdd(&ws.b.hdr[cur ^ 1], 1)] = e;
        return;
    }
    const int R = nrules[e], d = ws.b.d[e], K = ws.K[e];
    if (tid == 0)
        bits_s = rw_walk_starts(d, K, STEPPED ? n : K, STEPPED, ws.b.steps + rows0, ws.b.reward + rows0, ws.used + en, ws.steps_inc + en, ws.prev + en,
                                good_above, tol);
    __syncthreads();
    const uint32_t bits = bits_s;
    int Rn = R;
    if (bits)                                                          // uniform
        Rn = reduce_batch_compact<NANT>(rb + (size_t)e * (NANT + 1) * M, rant ? rant + (size_t)e * NANT * M : nullptr,
                                        uidx ? uidx + (size_t)e * NANT * M : nullptr, ws.b.alive + (size_t)e * M, ws.b.slot + (size_t)e * M, M, R, bits,
                                        wave_kept);
    __syncthreads();                                                   // every thread has read the agent's state
    if (tid != 0) return;
    ws.b.rounds[e] += 1;
    ws.b.rollouts[e] += rw_nodes(d) * K;
    nrules[e] = Rn;
    ws.b.prev[e] = ws.prev[en + ws.used[en]];
    const int j = ws.b.j[e] + d;
    ws.b.j[e] = j;
    if (j < ws.b.R0[e]) ws.b.live[cur ^ 1][atomicAdd(&ws.b.hdr[cur ^ 1], 1)] = e;
}

// prev_reward of every start that took a baseline replay, after the last accepted removal
__global__ void reduce_starts_result_kernel(int total, ReduceStartsWs ws)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (ws.steps_inc[i] >= 0) ws.res[i].reward = ws.prev[i];
}

}  // namespace frirl
