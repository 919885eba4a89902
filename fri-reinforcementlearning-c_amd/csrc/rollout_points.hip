// rollout_points.hip -- frirl_hip_rollout_points (include/frirl_hip.h): the roll-outs of frirl_hip_rollout_batch's
// tiled form, one episode per row, that keep per agent the de-duplicated SET of points the policy was asked at -- what
// frirl_hip_rollout_record + frirl_hip_log_points give, without a record ever being written.
//
// Launches of a call, nothing read back in between:
//   roll      a workgroup serves rows of ONE agent through shared_sweep (a COPY of the step loop of rollout_record_episodes.h with one
//             episode per row; one loop with a sink for both cost this kernel 0.7 %, profiles/r24_rollout_loop.md) and keeps the
//             points of its rows in an LDS hash table, each entry with the mask of the rows that visited it; when every row has
//             ended it writes the entries whose visitors include a contributing row to ITS segment of the workspace
//   finalise  one workgroup per agent merges the segments of the agent's workgroups (bit-wise de-duplication against the list so
//             far, as log_points_dedup_kernel) into points / point_count / overflow, and gives the rows that were not rolled out
//             steps -1 / reward 0 / success 0
// No workgroup reads what another one wrote in the same launch: the segments change hands at the launch boundary.
#include "shared_sweep.h"
#include "envs.h"
#include "batch_shape.h"
#include "shape_ladder.h"
#include <type_traits>

namespace frirl {

// A workgroup's point table (open addressing, linear probing; 8 * ns + 8 bytes per slot of dynamic LDS) has 256 / 512 / 768 slots for
// cap <= 128 / 384 / 512 and takes slots - RP_SPARE >= cap entries, so a probe always ends at an empty slot: a smaller cap buys
// occupancy (nant 5: 28 / 38 / 48 KB of LDS per workgroup in all).
constexpr int RP_SPARE = 128;
__host__ __device__ inline int rp_slots(int cap) { return (cap + RP_SPARE + 255) / 256 * 256; }
constexpr int RP_MIN_ROWS = 4;                 // rows of a workgroup at least (G * H <= 64 lanes per row): what the segments are sized for

// header of a workgroup's segment, in front of its [cap][NS] rows
struct PointSegment {
    int32_t count;                             // rows written (<= cap)
    int32_t overflow;                          // 1 = the table filled up, or more than cap entries were to be kept
    int32_t pad[2];
};

__host__ __device__ inline size_t rp_segment_bytes(int ns, int cap) { return sizeof(PointSegment) + sizeof(uint64_t) * (size_t)ns * (size_t)cap; }

// rows of agent e that are rolled out.  The descriptor goes by reference on purpose: the roll kernel's registers depend on it
// (profiles/r24_rollout_loop.md, section 3).
__device__ __forceinline__ int points_rows(const frirl_hip_rollout_points_desc &rp, const int32_t *__restrict__ nrules, int maxR, int e)
{
    return agent_rows(rp.row_count, rp.active, rp.n, nrules, maxR, e);
}

template <int NS>
struct PointTable {
    uint64_t *key;                             // [slots][NS]
    unsigned long long *visitors;              // [slots] bit r = local row r asked the policy at this point; 0 = the slot is empty
    int slots;
};

template <int NS>
struct PointStage {
    uint64_t staged[SH_BLOCK / 4][NS];         // the misses of this step, by local row
    unsigned long long staged_rows;            // local rows with a staged miss
    unsigned long long good;                   // local rows whose episode contributes
    int entries, overflow;
    int wave_kept[SH_BLOCK / FRIRL_WAVE];
};

template <int NS>
__device__ __forceinline__ unsigned point_slot(const uint64_t (&x)[NS], int slots)
{
    uint64_t hsh = 0;
#pragma unroll
    for (int k = 0; k < NS; k++) hsh = (hsh ^ x[k]) * 0x9E3779B97F4A7C15ull;
    return (unsigned)(hsh >> 40) % (unsigned)slots;
}

// slot of x, or of the empty slot its probe ends at (`found` tells which)
template <int NS>
__device__ __forceinline__ unsigned point_find(const PointTable<NS> &pt, const uint64_t (&x)[NS], bool &found)
{
    unsigned s = point_slot<NS>(x, pt.slots);
    for (int i = 0; i < pt.slots; i++) {       // RP_SPARE slots stay empty: ends at one of them long before
        if (pt.visitors[s] == 0ull) { found = false; return s; }
        bool same = true;
#pragma unroll
        for (int k = 0; k < NS; k++) same = same && pt.key[(size_t)s * NS + k] == x[k];
        if (same) { found = true; return s; }
        s = s + 1 == (unsigned)pt.slots ? 0 : s + 1;
    }
    found = false;
    return s;
}

// `wpa` workgroups per agent, each serving 256 / (G * H) rows of that agent.  All conditions in front of the barriers are uniform over
// the workgroup: they depend on the agent and on the workgroup's first row only.  The table is written in two places that barriers keep
// apart: by the group leaders' atomic OR on an entry that exists, between the loop's barrier and shared_sweep's first one (the keys are
// only read there), and by thread 0, which inserts the staged misses in local-row order behind shared_sweep's last barrier and in
// front of the loop's (nobody else touches the table there).
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void rollout_points_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                   const double *__restrict__ rb_all, const int32_t *__restrict__ nrules, int maxR,
                                                                   const frirl_hip_agent ag, int wpa, int segs, const frirl_hip_rollout_points_desc rp,
                                                                   char *__restrict__ segments)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    static_assert(EPB <= 64 && EPB <= SH_BLOCK / 4, "one visitor bit and one staging row per local row");
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    __shared__ PointStage<NS> st;
    extern __shared__ unsigned long long point_table[];              // [slots][NS] keys, [slots] visitors
    PointTable<NS> pt;
    pt.slots = rp_slots(rp.cap);
    pt.key = reinterpret_cast<uint64_t *>(point_table);
    pt.visitors = point_table + (size_t)pt.slots * NS;
    const int e = (int)(blockIdx.x / (unsigned)wpa), wg = (int)(blockIdx.x % (unsigned)wpa);
    const int row0 = wg * EPB;
    const int rows = points_rows(rp, nrules, maxR, e);
    if (row0 >= rows || wg >= segs) return;                          // nothing to roll out here (wg < segs by the host's arithmetic)
    const int lrow = threadIdx.x / GH, j = row0 + lrow;
    const bool exists = j < rows;
    const size_t q = (size_t)e * rp.n + (exists ? j : 0);
    using POW = KernelPow<NANT, PN>;
    POW p = kernel_pow<NANT, PN>(ag);
    const double *rb = rb_all + (size_t)e * (NANT + 1) * maxR;
    const int R = nrules[e];

    const GroupLane l = group_lane<G, H, AMAX>(ag.A);
    const bool leader = l.leader;
    stage_agent<NANT>(tl, grid_s, ag);
    for (int i = threadIdx.x; i < pt.slots; i += SH_BLOCK) pt.visitors[i] = 0ull;
    if (threadIdx.x == 0) { st.staged_rows = 0ull; st.good = 0ull; st.entries = 0; st.overflow = 0; }
    const unsigned long long mybit = 1ull << lrow;
    double states[NS], cur[NS], qs[NS], qv[NS], total = 0.0, action = 0.0;
    uint64_t last[NS];                                               // the point this row asked at last: it carries the row's bit already
#pragma unroll
    for (int k = 0; k < NS; k++) { states[k] = 0.0; cur[k] = 0.0; qs[k] = 0.0; qv[k] = 0.0; last[k] = 0; }
    int steps = 0, success = 0;
    bool fresh = true, fin = !exists, have_last = false;
    for (;;) {
        if (__syncthreads_count(fin ? 0 : 1) == 0) break;            // every row of the workgroup has ended; also: the table is initialised / complete
        double r = 0.0;
        if (!fin) {
            if (fresh) {
                const double *start = rp.start_states ? rp.start_states + q * NS : nullptr;
#pragma unroll
                for (int k = 0; k < NS; k++) {
                    states[k] = start ? start[k] : ag.values_def[k];                                     // frirl_episode.c:46-48
                    qv[k] = observe_ve(u, ve, U, k, states[k]);
                }
            } else {
                env_do_action(ag.env_kind, action, states, cur);                                         // :97
                env_get_reward(ag.env_kind, cur, r, success);                                            // :106
                total = total + r;                                                                       // :107
                env_quantize(ag.env_kind, NS, grid_s, ag.grid_len, ag.grid_div, cur, qs);                // :112
#pragma unroll
                for (int k = 0; k < NS; k++) qv[k] = observe_ve(u, ve, U, k, qs[k]);
            }
            if (leader) {                                            // the point of this step: the un-quantised start, else q_obs
                uint64_t x[NS];
                bool again = have_last;
#pragma unroll
                for (int k = 0; k < NS; k++) {
                    x[k] = (uint64_t)__double_as_longlong(fresh ? states[k] : qs[k]);
                    again = again && x[k] == last[k];
                }
                if (!again) {
                    bool found;
                    const unsigned s = point_find<NS>(pt, x, found);
                    if (found) {
                        if (!(pt.visitors[s] & mybit)) atomicOr(&pt.visitors[s], mybit);
                    } else {
#pragma unroll
                        for (int k = 0; k < NS; k++) st.staged[lrow][k] = x[k];
                        atomicOr(&st.staged_rows, mybit);
                    }
#pragma unroll
                    for (int k = 0; k < NS; k++) last[k] = x[k];
                    have_last = true;
                }
            }
        }
        unsigned h0;
        int pa;
        double bv;
        shared_sweep<NANT, AMAX, true, false, G, H, POW>(tl, rb, nullptr, R, maxR, p, l.abeg, l.aend, l.nchunks, qv, !fin, 0u, nullptr, h0, pa, bv, l.h);   // :78 / :148
        group_first_max<G>(bv, pa);
        if (threadIdx.x == 0) {                                      // the serial phase: this step's misses, in local-row order
            unsigned long long todo = st.staged_rows;
            if (todo) st.staged_rows = 0ull;
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                uint64_t x[NS];
#pragma unroll
                for (int k = 0; k < NS; k++) x[k] = st.staged[l][k];
                bool found;
                const unsigned s = point_find<NS>(pt, x, found);     // an earlier row of this phase may have brought the same point
                if (found) { pt.visitors[s] |= 1ull << l; continue; }
                if (st.entries >= pt.slots - RP_SPARE) { st.overflow = 1; continue; }
#pragma unroll
                for (int k = 0; k < NS; k++) pt.key[(size_t)s * NS + k] = x[k];
                pt.visitors[s] = 1ull << l;
                st.entries++;
            }
        }
        if (!fin) {
            bool ended;
            if (fresh) {
                pa = e_greedy(ag, pa, (uint32_t)q, 0u, 0u);
                fresh = false;
                ended = ag.max_steps < 1;                                                                // :86
            } else {
                steps++;                                                                                 // :174
                pa = e_greedy(ag, pa, (uint32_t)q, 0u, (uint32_t)steps);
#pragma unroll
                for (int k = 0; k < NS; k++) states[k] = cur[k];                                         // :163-165
                ended = success == 1 || steps >= ag.max_steps;                                           // :183, :86
            }
            action = grid_s[NS * FRIRL_HIP_MAX_GRID + pa];                                               // :82 / :151
            if (ended) {
                fin = true;
                if (leader) {
                    if (rp.steps) rp.steps[q] = steps;
                    if (rp.reward) rp.reward[q] = total;
                    if (rp.success) rp.success[q] = success;
                    if (!rp.only_successful || success == 1) atomicOr(&st.good, mybit);
                }
            }
        }
    }
    // ---- flush: the entries a contributing row visited, in slot order, to this workgroup's segment ------------------------------
    char *seg = segments + ((size_t)e * segs + wg) * rp_segment_bytes(NS, rp.cap);
    uint64_t *out = reinterpret_cast<uint64_t *>(seg + sizeof(PointSegment));
    const unsigned long long good = st.good;
    int count = 0, over = st.overflow;                               // the same in every thread
    for (int s0 = 0; s0 < pt.slots; s0 += SH_BLOCK) {                // slots is a multiple of the workgroup
        const int s = s0 + threadIdx.x;
        const bool keep = (pt.visitors[s] & good) != 0ull;
        const int pos = block_append<SH_BLOCK>(keep, st.wave_kept, rp.cap, count, over);
        if (keep && pos < rp.cap) {
#pragma unroll
            for (int k = 0; k < NS; k++) out[(size_t)pos * NS + k] = pt.key[(size_t)s * NS + k];
        }
        __syncthreads();                                            // wave_kept is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        PointSegment *hd = reinterpret_cast<PointSegment *>(seg);
        hd->count = count;
        hd->overflow = over;
    }
}

constexpr int RPF_BLOCK = 256;

// Finalise: one workgroup per agent.  The candidates (segment ascending, row ascending) are taken 256 at a time: a candidate is new iff
// no point of the list so far equals it bit-wise (the rows of ONE segment are distinct already, so a chunk holds no duplicates of its
// own and the first segment needs no comparison); the new ones are appended in candidate order.
template <int NS>
__global__ __launch_bounds__(RPF_BLOCK) void rollout_points_finalise_kernel(const int32_t *__restrict__ nrules, int maxR, int epb, int segs,
                                                                             const frirl_hip_rollout_points_desc rp, const char *__restrict__ segments)
{
    __shared__ int wave_new[RPF_BLOCK / FRIRL_WAVE];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int rows = points_rows(rp, nrules, maxR, e);
    for (int j = rows + tid; j < rp.n; j += RPF_BLOCK) {              // the rows that were not rolled out
        const size_t q = (size_t)e * rp.n + j;
        if (rp.steps) rp.steps[q] = -1;
        if (rp.reward) rp.reward[q] = 0.0;
        if (rp.success) rp.success[q] = 0;
    }
    int used = (rows + epb - 1) / epb;                                // workgroups of this agent that wrote a segment
    used = used > segs ? segs : used;
    uint64_t *list = reinterpret_cast<uint64_t *>(rp.points) + (size_t)e * rp.cap * NS;
    int count = 0, over = 0;                                          // the same in every thread
    for (int sg = 0; sg < used; sg++) {
        const char *seg = segments + ((size_t)e * segs + sg) * rp_segment_bytes(NS, rp.cap);
        const PointSegment *hd = reinterpret_cast<const PointSegment *>(seg);
        const uint64_t *src = reinterpret_cast<const uint64_t *>(seg + sizeof(PointSegment));
        int n = hd->count;
        n = n < 0 ? 0 : (n > rp.cap ? rp.cap : n);
        over |= hd->overflow != 0 ? 1 : 0;
        const int before = count;                                     // the list in front of this segment
        for (int c0 = 0; c0 < n; c0 += RPF_BLOCK) {
            const int c = c0 + tid;
            uint64_t x[NS] = {};
            bool fresh = c < n;
            if (fresh) {
#pragma unroll
                for (int k = 0; k < NS; k++) x[k] = src[(size_t)c * NS + k];
            }
            for (int i = 0; fresh && i < before; i++) {
                bool same = true;
#pragma unroll
                for (int k = 0; k < NS; k++) same = same && list[(size_t)i * NS + k] == x[k];
                fresh = !same;
            }
            const int pos = block_append<RPF_BLOCK>(fresh, wave_new, rp.cap, count, over);
            if (fresh && pos < rp.cap) {
#pragma unroll
                for (int k = 0; k < NS; k++) list[(size_t)pos * NS + k] = x[k];
            }
            __syncthreads();                                         // wave_new is rewritten by the next chunk; the rows written are visible
        }
    }
    if (tid == 0) { rp.point_count[e] = count; rp.overflow[e] = over; }
}

}  // namespace frirl

using namespace frirl_host;

namespace {

// segments per agent the workspace is sized for: a workgroup serves RP_MIN_ROWS rows at least, whatever the lane shape
size_t points_segments(size_t n) { return (n + frirl::RP_MIN_ROWS - 1) / frirl::RP_MIN_ROWS; }

template <int N, int AMAX, int G, int H, bool PN>
void launch_points(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_points_desc *rp, char *segments,
                   hipStream_t s)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    static_assert(EPB >= frirl::RP_MIN_ROWS, "the workspace holds a segment per RP_MIN_ROWS rows");
    const int wpa = (rp->n + EPB - 1) / EPB, segs = (int)points_segments((size_t)rp->n);
    const size_t table = sizeof(uint64_t) * (size_t)frirl::rp_slots(rp->cap) * N;      // N - 1 key words and the visitors per slot
    hipLaunchKernelGGL((frirl::rollout_points_kernel<N, AMAX, G, H, PN>), dim3((unsigned)b->E * (unsigned)wpa), dim3(frirl::SH_BLOCK), table, s, t->u, t->ve,
                       t->U, b->rb, b->nrules, b->maxR, *ag, wpa, segs, *rp, segments);
    hipLaunchKernelGGL((frirl::rollout_points_finalise_kernel<N - 1>), dim3((unsigned)b->E), dim3(frirl::RPF_BLOCK), 0, s, b->nrules, b->maxR, EPB, segs, *rp,
                       segments);
}

template <int N>
void launch_points_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_points_desc *rp, char *segments,
                     hipStream_t s)
{
    frirl::for_batch_shape<N>(ag, rb_rollout_slices(b->E, rp->n, ag->A, opts().rollout_points_slices), [&](auto sh) {
        using S = decltype(sh);
        launch_points<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, rp, segments, s);
    });
}

}  // namespace

extern "C" size_t frirl_hip_rollout_points_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t n, int32_t cap, int32_t A)
{
    if (nant < 2 || E < 1 || maxR < 1 || n < 1 || cap < 1 || A < 1) return 0;
    return up16((size_t)E * points_segments((size_t)n) * frirl::rp_segment_bytes(nant - 1, cap));
}

extern "C" int frirl_hip_rollout_points(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                        const frirl_hip_rollout_points_desc *rp, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *who = "frirl_hip_rollout_points";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if ((rc = check_rollout_agent_null(agent, rp != nullptr, who))) return rc;
    if (!rp->points || !rp->point_count || !rp->overflow) { set_error("%s: NULL points / point_count / overflow", who); return FRIRL_HIP_EINVAL; }
    if (rp->n < 1 || rp->n > FRIRL_HIP_REDUCE_MAX_STARTS) { set_error("%s: n=%d outside 1..%d", who, rp->n, FRIRL_HIP_REDUCE_MAX_STARTS); return FRIRL_HIP_EINVAL; }
    if (rp->cap < 1 || rp->cap > FRIRL_HIP_POINTS_MAX_CAP) { set_error("%s: cap=%d outside 1..%d", who, rp->cap, FRIRL_HIP_POINTS_MAX_CAP); return FRIRL_HIP_EINVAL; }
    if (rp->only_successful != 0 && rp->only_successful != 1) { set_error("%s: only_successful=%d is not 0 / 1", who, rp->only_successful); return FRIRL_HIP_EINVAL; }
    if ((int64_t)b->E * rp->n > INT32_MAX || (int64_t)b->E * rp->cap > INT32_MAX) {
        set_error("%s: E * n = %lld rows or E * cap = %lld points exceed INT32_MAX", who, (long long)b->E * rp->n, (long long)b->E * rp->cap);
        return FRIRL_HIP_EINVAL;
    }
    if ((rc = check_rollout_agent(t, agent, who))) return rc;
    const size_t need = frirl_hip_rollout_points_workspace_bytes(t->nant, b->E, b->maxR, rp->n, rp->cap, agent->A);
    if ((rc = check_workspace(who, workspace, workspace_bytes, need, "frirl_hip_rollout_points_workspace_bytes")) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    if (t->nant == 3) launch_points_n<3>(t, b, agent, rp, static_cast<char *>(workspace), s);
    else launch_points_n<5>(t, b, agent, rp, static_cast<char *>(workspace), s);
    return check_launch(who);
}
