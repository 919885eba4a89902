// reduce_batch.hip -- the rule-base reduction (frirl_sequential_run.c:170-350) of EVERY rule base of a batch in one run of
// speculative try-remove rounds (frirl_hip_reduce_batch; include/frirl_hip.h, DESIGN.md "Batched reduction").
//
// A round is three launches over the agents that are still reducing (the live list, built on the device):
//   open   slot table of the next d_e = min(depth, R0_e - j_e) candidates of every live agent
//   roll   one replay per node of every live agent's accept/reject tree; a workgroup serves rows of ONE agent and points
//          rollout_episode / shared_sweep (the code of frirl_hip_rollout_shared) at that agent's slab, start state and step cap
//   close  tree walk (reduce_walk.h), in-place compaction of the agent's columns, next live list
// and the host reads one 16-byte header (the live count) per round.  No slab and no per-row result crosses to the host.
#include "rollout_episode.h"
#include "reduce_walk.h"
#include <cstring>
#include <type_traits>

namespace frirl {

constexpr int RB_ORDER_TILE = 1024;      // |Q| values staged in LDS per pass of the rank count

// the arrays of one call, carved out of the caller's workspace (reduce_batch_layout)
struct ReduceBatchWs {
    int32_t *hdr;                 // [4] live count of even rounds, of odd rounds, first agent with a bad rule count + 1, pad
    uint32_t *mask;               // [nodes] exclude mask of every tree node: the same for every agent
    int32_t *live[2];             // [E] agents still reducing, this round's list and the next one's
    int32_t *order;               // [E][maxR] candidates in trial order (original rule indices)
    int32_t *alive;               // [E][maxR] original index of the rule in each current slot
    uint8_t *slot;                // [E][maxR] candidate slot of every current rule in this round, 255 = none
    int32_t *steps;               // [E][nodes] replay results of this round
    double *reward;               // [E][nodes]
    int32_t *j, *d, *R0, *rounds, *rollouts, *steps_inc, *cap;      // [E]
    double *prev;                 // [E] prev_reward
    frirl_hip_reduce_result *res; // [E]
    int nodes;                    // 2^depth - 1
};

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

// Batched roll-out kernel: `wpa` workgroups per live agent, each serving 256 / (G * H) nodes of that agent's tree (first: the
// baseline replay, one row per agent, no exclusions).  All conditions in front of the barriers are uniform over the workgroup:
// they depend on the agent and on the workgroup's first row only.
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void reduce_batch_rollout_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                         const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                         const frirl_hip_agent ag, const double *__restrict__ start_states, int cur,
                                                                         int wpa, int first, ReduceBatchWs ws)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int e = ws.live[cur][blockIdx.x / wpa];
    const int row0 = (blockIdx.x % wpa) * EPB;
    const int n = first ? 1 : rw_nodes(ws.d[e]);
    if (row0 >= n) return;                                             // the whole workgroup, before the first barrier
    const int node = row0 + threadIdx.x / GH;
    const bool exists = node < n;                                      // nodes with k >= d_e do not exist
    const uint32_t mask = (exists && !first) ? ws.mask[node] : 0u;
    using POW = typename std::conditional<PN, PowC<NANT>, PowU>::type;
    POW p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;
    double states[NS], total;
    int steps, success;
    rollout_episode<NANT, AMAX, G, H, true, POW>(tl, grid_s, u, ve, U, rb + (size_t)e * (NANT + 1) * maxR, ws.slot + (size_t)e * maxR, nrules[e], maxR, ag, p,
                                                  exists, (uint32_t)node, mask, start_states ? start_states + (size_t)e * NS : nullptr, ws.cap[e], steps,
                                                  total, success, states);
    if (!exists || threadIdx.x % GH != 0) return;
    ws.steps[(size_t)e * ws.nodes + node] = steps;
    ws.reward[(size_t)e * ws.nodes + node] = total;
}

// Close-round kernel: one workgroup per live agent.  first: the baseline replay sets steps_incremental, prev_reward and the
// agent's step cap.  Otherwise: walk the tree (every thread, same result), compact the rule base in place -- chunks of 256 rules
// in index order, every chunk read into registers by all threads before any of it is written, and a write never lands above
// its read -- zero the vacated tail, advance the agent and append it to the next live list while candidates are left.
template <int NANT>
__global__ __launch_bounds__(256) void reduce_batch_close_kernel(double *__restrict__ rb, int32_t *__restrict__ nrules, uint16_t *__restrict__ uidx,
                                                                 double *__restrict__ rant, int maxR, int cur, int first, int max_steps,
                                                                 double good_above, double tol, ReduceBatchWs ws)
{
    __shared__ int wave_kept[4];
    const int e = ws.live[cur][blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t M = (size_t)maxR;
    const int R = nrules[e], d = first ? 0 : ws.d[e];
    const int steps_inc = first ? ws.steps[(size_t)e * ws.nodes] : ws.steps_inc[e];
    double prev = first ? ws.reward[(size_t)e * ws.nodes] : ws.prev[e];
    const uint32_t bits = rw_walk(d, ws.steps + (size_t)e * ws.nodes, ws.reward + (size_t)e * ws.nodes, steps_inc, prev, good_above, tol);
    int Rn = R;
    if (bits) {                                                        // uniform: every thread walked the same tree
        double *cols = rb + (size_t)e * (NANT + 1) * M;
        double *ra = rant ? rant + (size_t)e * NANT * M : nullptr;
        uint16_t *ui = uidx ? uidx + (size_t)e * NANT * M : nullptr;
        int32_t *al = ws.alive + (size_t)e * M;
        const uint8_t *sl = ws.slot + (size_t)e * M;
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
        Rn = base;
        for (int r = Rn + tid; r < R; r += 256) {                      // vacated tail: zero like five_remove_rule.c:64-80
#pragma unroll
            for (int k = 0; k <= NANT; k++) cols[k * M + r] = 0.0;
#pragma unroll
            for (int k = 0; k < NANT; k++) { if (ra) ra[k * M + r] = 0.0; if (ui) ui[k * M + r] = 0; }
        }
    }
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

using namespace frirl_host;
using frirl::ReduceBatchWs;

// ---- shapes ----------------------------------------------------------------------------------------------------------------
// Lanes per row: G action slots (4 for up to 4 actions, else 8) times H rule slices.  The rounds run H = 8 while that keeps every
// row resident, the baseline replay (one row per agent) the widest group a wave holds.
static constexpr int RB_H = 8;              // rule slices of the shape the depth rule counts with

static int rb_group(int A) { return A <= 4 ? 4 : 8; }

// Resident workgroups per CU of the H = 8 roll-out kernels (one wave of a workgroup per SIMD, so = waves per SIMD), from their
// register counts: G = 4 needs 107 (nant 3) / 133 (nant 5) VGPRs -> 4 / 3 waves, G = 8 needs 235 / 255 -> 2 / 1.  The
// smaller of the two antecedent counts is taken; the 15.6 KB of LDS per workgroup would allow 10.
static int rb_wg_per_cu(int A) { return A <= 4 ? 3 : 1; }

static int rb_cus()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) return n;
    (void)hipGetLastError();
    return 256;                              // no device visible: an MI355X is assumed
}

// rows the H = 8 shape keeps resident on the chip
static long rb_resident_rows(int A) { return (long)rb_cus() * rb_wg_per_cu(A) * (frirl::SH_BLOCK / (rb_group(A) * RB_H)); }

extern "C" int frirl_hip_reduce_batch_depth(int32_t E, int32_t A)
{
    if (E < 1) E = 1;
    const long rows = rb_resident_rows(A);
    int d = 1;
    while (d < 10 && (long)E * frirl::rw_nodes(d + 1) <= rows) d++;
    return d;
}

static size_t up16(size_t n) { return (n + 15) / 16 * 16; }

// carves the arrays of a call out of `base` (NULL: sizes only); `rows` = entries of steps / reward
static size_t reduce_batch_layout(char *base, size_t E, size_t maxR, int depth, size_t rows, ReduceBatchWs *ws)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    ReduceBatchWs w;
    w.nodes = frirl::rw_nodes(depth);
    w.hdr = reinterpret_cast<int32_t *>(take(4 * sizeof(int32_t)));
    w.mask = reinterpret_cast<uint32_t *>(take(sizeof(uint32_t) * w.nodes));
    w.live[0] = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.live[1] = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.order = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * maxR));
    w.alive = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * maxR));
    w.slot = reinterpret_cast<uint8_t *>(take(E * maxR));
    w.steps = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * rows));
    w.reward = reinterpret_cast<double *>(take(sizeof(double) * rows));
    int32_t **per_agent[] = {&w.j, &w.d, &w.R0, &w.rounds, &w.rollouts, &w.steps_inc, &w.cap};
    for (int32_t **p : per_agent) *p = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.prev = reinterpret_cast<double *>(take(sizeof(double) * E));
    w.res = reinterpret_cast<frirl_hip_reduce_result *>(take(sizeof(frirl_hip_reduce_result) * E));
    if (ws) *ws = w;
    return off;
}

extern "C" size_t frirl_hip_reduce_batch_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t depth)
{
    (void)nant;                              // no array of the workspace depends on it
    if (E < 1 || maxR < 1 || depth < 0 || depth > frirl::RW_MAX_DEPTH) return 0;
    if (depth > 0) return reduce_batch_layout(nullptr, E, maxR, depth, (size_t)E * frirl::rw_nodes(depth), nullptr);
    // depth 0: the depth frirl_hip_reduce_batch_depth selects is not known without the action count -- enough for any (the shape of
    // up to 4 actions holds the most rows), and never less for more agents
    const long cap = rb_resident_rows(1);
    return reduce_batch_layout(nullptr, E, maxR, 10, (size_t)((long)E > cap ? (long)E : cap), nullptr);
}

template <int N, int AMAX, int G, int H, bool PN = true>
static void launch_rows(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const double *start, int cur, int nlive,
                        int nodes, int first, const ReduceBatchWs &ws, hipStream_t s)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    const int wpa = (nodes + EPB - 1) / EPB;
    hipLaunchKernelGGL((frirl::reduce_batch_rollout_kernel<N, AMAX, G, H, PN>), dim3((unsigned)nlive * wpa), dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb,
                       b->nrules, b->maxR, *ag, start, cur, wpa, first, ws);
}

// rule slices of a round with `rows` rows in all: 8 while every row stays resident, else 4, else 1
static int rb_slices(long rows, int A)
{
    const long rows8 = rb_resident_rows(A);
    return rows <= rows8 ? 8 : (rows <= 2 * rows8 ? 4 : 1);
}

template <int N>
static void launch_rows_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const double *start, int cur, int nlive,
                          int nodes, int first, const ReduceBatchWs &ws, hipStream_t s)
{
    const bool few = ag->A <= 4;
    if (ag->p > 0 && ag->p != N) {          // run-time Shepard power: the variants without rule slices, as frirl_hip_rollout_shared
        if (few) launch_rows<N, 1, 4, 1, false>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else launch_rows<N, 4, 8, 1, false>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        return;
    }
    const int H = first ? (few ? 16 : 8) : rb_slices((long)nlive * nodes, ag->A);
    if (few) {
        if (H == 16) launch_rows<N, 1, 4, 16>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else if (H == 8) launch_rows<N, 1, 4, 8>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else if (H == 4) launch_rows<N, 1, 4, 4>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else launch_rows<N, 1, 4, 1>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
    } else {
        if (H == 8) launch_rows<N, 4, 8, 8>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else if (H == 4) launch_rows<N, 4, 8, 4>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
        else launch_rows<N, 4, 8, 1>(t, b, ag, start, cur, nlive, nodes, first, ws, s);
    }
}

extern "C" int frirl_hip_reduce_walk_check(int d, const int32_t *steps, const double *reward, int steps_inc, double prev_reward, double good_above,
                                           double tol, uint32_t *bits_out, double *prev_out)
{
    if (d < 0 || d > frirl::RW_MAX_DEPTH || (d > 0 && (!steps || !reward)) || !bits_out || !prev_out) {
        set_error("frirl_hip_reduce_walk_check: d=%d outside 0..%d or NULL argument", d, frirl::RW_MAX_DEPTH);
        return FRIRL_HIP_EINVAL;
    }
    double prev = prev_reward;
    *bits_out = frirl::rw_walk(d, steps, reward, steps_inc, prev, good_above, tol);
    *prev_out = prev;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reduce_batch(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                      const double *start_states, const uint8_t *active, int strategy, double reward_tolerance, int depth,
                                      int32_t *kept, frirl_hip_reduce_result *results, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_reduce_batch";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!agent || !results || !agent->grid_values || !agent->action_ve) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (strategy != 1 && strategy != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy); return FRIRL_HIP_EINVAL; }
    if (depth < 0 || depth > frirl::RW_MAX_DEPTH) { set_error("%s: depth %d outside 0..%d", who, depth, frirl::RW_MAX_DEPTH); return FRIRL_HIP_EINVAL; }
    if (agent->A < 1 || agent->A > FRIRL_HIP_MAX_ACTIONS || agent->max_steps < 0) { set_error("%s: A=%d / max_steps=%d out of range", who, agent->A, agent->max_steps); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, who))) return rc;
    for (int k = 0; k < t->nant; k++)
        if (agent->grid_len[k] < 1 || agent->grid_len[k] > FRIRL_HIP_MAX_GRID) { set_error("%s: grid_len[%d]=%d outside 1..%d", who, k, agent->grid_len[k], FRIRL_HIP_MAX_GRID); return FRIRL_HIP_EINVAL; }
    if (depth == 0) depth = frirl_hip_reduce_batch_depth(b->E, agent->A);
    const size_t E = (size_t)b->E, M = (size_t)b->maxR;
    const int nodes = frirl::rw_nodes(depth);
    const size_t need = reduce_batch_layout(nullptr, E, M, depth, E * nodes, nullptr);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need) {
        set_error("%s: workspace %p / %zu bytes: needs %zu bytes, 16-byte aligned (frirl_hip_reduce_batch_workspace_bytes)", who, workspace, workspace_bytes, need);
        return FRIRL_HIP_EINVAL;
    }
    if ((rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
#define RB_TRY(expr)                                                                                               \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) { set_error("%s: %s: %s", who, #expr, hipGetErrorString(e_)); return FRIRL_HIP_ELAUNCH; } \
    } while (0)
    ReduceBatchWs ws;
    reduce_batch_layout(static_cast<char *>(workspace), E, M, depth, E * nodes, &ws);
    frirl_hip_agent greedy = *agent;
    greedy.no_random = 1;                                             // the replays are greedy (reduction_state == 1 keeps epsilon at 0 in every demo)
    int32_t hdr[4] = {0, 0, 0, 0};
    RB_TRY(hipMemsetAsync(ws.hdr, 0, sizeof hdr, s));
    hipLaunchKernelGGL(frirl::reduce_batch_order_kernel, dim3((unsigned)E), dim3(256), 0, s, b->rb, b->nrules, t->nant, b->maxR, active, strategy,
                       greedy.max_steps, ws);
    RB_TRY(hipMemcpyAsync(hdr, ws.hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
    RB_TRY(hipStreamSynchronize(s));
    if (hdr[2]) { set_error("%s: agent %d: nrules outside 1..maxR=%d", who, hdr[2] - 1, b->maxR); return FRIRL_HIP_EINVAL; }
    // round 0 = the baseline replay of every active agent (:196-198 and the first loop iteration, :204-206); then rounds until no
    // agent has a candidate left.  Per round the host reads the 16-byte header: the next round's live count.
    for (int round = 0;; round++) {
        const int cur = round & 1, first = round == 0;
        const int nlive = hdr[cur];
        if (nlive == 0) break;
        if (!first) hipLaunchKernelGGL(frirl::reduce_batch_open_kernel, dim3(nlive), dim3(256), 0, s, b->nrules, b->maxR, depth, cur, ws);
        if (t->nant == 3) launch_rows_n<3>(t, b, &greedy, start_states, cur, nlive, first ? 1 : nodes, first, ws, s);
        else launch_rows_n<5>(t, b, &greedy, start_states, cur, nlive, first ? 1 : nodes, first, ws, s);
        if (t->nant == 3)
            hipLaunchKernelGGL(frirl::reduce_batch_close_kernel<3>, dim3(nlive), dim3(256), 0, s, b->rb, b->nrules, b->uidx, rant, b->maxR, cur, first,
                               greedy.max_steps, agent->reward_good_above, reward_tolerance, ws);
        else
            hipLaunchKernelGGL(frirl::reduce_batch_close_kernel<5>, dim3(nlive), dim3(256), 0, s, b->rb, b->nrules, b->uidx, rant, b->maxR, cur, first,
                               greedy.max_steps, agent->reward_good_above, reward_tolerance, ws);
        RB_TRY(hipMemcpyAsync(hdr, ws.hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
        RB_TRY(hipStreamSynchronize(s));
    }
    hipLaunchKernelGGL(frirl::reduce_batch_result_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, b->nrules, (int)E, ws);
    RB_TRY(hipMemcpyAsync(results, ws.res, sizeof(frirl_hip_reduce_result) * E, hipMemcpyDeviceToHost, s));
    if (kept) RB_TRY(hipMemcpyAsync(kept, ws.alive, sizeof(int32_t) * E * M, hipMemcpyDeviceToHost, s));
    RB_TRY(hipStreamSynchronize(s));
#undef RB_TRY
    return check_launch(who);
}
