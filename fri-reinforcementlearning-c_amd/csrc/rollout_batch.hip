// rollout_batch.hip -- frirl_test_run's greedy episode (frirl_episode.c:28-194 without the update at :155) for n rows on EVERY agent's
// own rule base in one call: frirl_hip_rollout_batch (include/frirl_hip.h, DESIGN.md "Batched roll-outs").  Row q = e * n + j runs on
// the slab of agent e = q / n, exactly what frirl_hip_rollout_shared does on that slab alone with the row's start state.
//
// Launches of a call, nothing read back in between:
//   prep      per-agent row count (0 for an agent that is inactive or whose nrules lies outside 1..maxR), step cap and row counter;
//             the rows that are not rolled out get steps -1, reward 0, success 0
//   resident  agents whose rule base fits the LDS image of rollout_resident.h: `wpa` workgroups per agent stage the agent's image and
//             hash table ONCE, then groups of H lanes take the agent's rows one after another from the agent's counter; no barrier
//             and no re-staging per step.  The workgroups of an agent that does not fit return before staging
//   tiled     the agents the resident form did not serve (decided by the same comparison on the device): a workgroup serves rows of
//             ONE agent through rollout_episode / shared_sweep, as the batched reduction's roll-out kernel does
//   score     per agent, from the per-row outputs in row order
#include "rollout_episode.h"
#include "rollout_resident.h"
#include "batch_shape.h"
#include "shape_ladder.h"
#include <type_traits>

namespace frirl {

constexpr int RBR_BLOCK = 256;     // threads of a resident workgroup at most (a launch may use 64, 128 or 192)

struct RolloutBatchWs {
    int32_t *rows;                 // [E] rows of the agent that are rolled out
    int32_t *cap;                  // [E] step cap
    uint32_t *next;                // [E] next row of the agent (resident form)
};

__global__ __launch_bounds__(256) void rollout_batch_prep_kernel(const int32_t *__restrict__ nrules, int E, int maxR, int max_steps,
                                                                 const frirl_hip_rollout_batch_rows ro, RolloutBatchWs ws)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)E * ro.n) return;
    const int e = (int)(q / ro.n), j = (int)(q - (long)e * ro.n);
    const int rows = agent_rows(ro.row_count, ro.active, ro.n, nrules, maxR, e);
    if (j == 0) {
        int cap = ro.step_cap ? ro.step_cap[e] : max_steps;
        cap = cap < 1 ? 1 : cap;
        ws.rows[e] = rows;
        ws.cap[e] = cap > max_steps ? max_steps : cap;
        ws.next[e] = 0u;
    }
    if (j >= rows) {
        ro.steps[q] = -1;
        ro.reward[q] = 0.0;
        if (ro.success) ro.success[q] = 0;
    }
}

// Tiled form: `wpa` workgroups per agent, each serving 256 / (G * H) rows of that agent.  All conditions in front of the barriers are
// uniform over the workgroup: they depend on the agent and on the workgroup's first row only.
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void rollout_batch_tiled_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                        const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                        const frirl_hip_agent ag, int wpa, int resident_rules,
                                                                        const frirl_hip_rollout_batch_rows ro, RolloutBatchWs ws)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int e = (int)(blockIdx.x / (unsigned)wpa);
    const int row0 = (int)(blockIdx.x % (unsigned)wpa) * EPB;
    const int rows = ws.rows[e];
    const int R = nrules[e];
    if (row0 >= rows || R <= resident_rules) return;                   // nothing to roll out here / the resident form served this agent
    const int j = row0 + threadIdx.x / GH;
    const bool exists = j < rows;
    const size_t q = (size_t)e * ro.n + (exists ? j : 0);
    double states[NS], total;
    int steps, success;
    rollout_episode<NANT, AMAX, G, H, false, KernelPow<NANT, PN>>(tl, grid_s, u, ve, U, rb + (size_t)e * (NANT + 1) * maxR, nullptr, R, maxR, ag,
                                                                   kernel_pow<NANT, PN>(ag), exists, (uint32_t)q, 0u,
                                                                   ro.start_states ? ro.start_states + q * NS : nullptr, ws.cap[e], steps, total, success, states);
    if (!exists || threadIdx.x % GH != 0) return;
    ro.steps[q] = steps;
    ro.reward[q] = total;
    if (ro.success) ro.success[q] = success;
    if (ro.final_states)
        for (int k = 0; k < NS; k++) ro.final_states[q * NS + k] = states[k];
}

struct ResidentBatchShape {
    int rps;                       // rules per column of the LDS image
    int ht;                        // slots of the exact-hit hash table (power of two >= 2 rps)
    int wpa;                       // workgroups per agent
};

// Resident form.  The loop of rollout_resident_kernel (rollout.hip) without its stages: a group never parks an episode, a
// never-succeeding episode holds its lanes to the step cap.
template <int NANT, int NA, int KIND, int H>
__global__ __launch_bounds__(RBR_BLOCK, 2) void rollout_batch_resident_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                               const double *__restrict__ rb_all, const int32_t *__restrict__ nrules, int maxR,
                                                                               const frirl_hip_agent ag, const ResidentBatchShape sh, int resident_rules,
                                                                               const frirl_hip_rollout_batch_rows ro, RolloutBatchWs ws)
{
    constexpr int NS = NANT - 1;
    extern __shared__ __attribute__((aligned(16))) double col[];       // [rps][NANT+1] rule base image (rule-major), [2][NANT][U] tables, hash table
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int nthr = (int)blockDim.x;
    const int e = (int)(blockIdx.x / (unsigned)sh.wpa), wg = (int)(blockIdx.x % (unsigned)sh.wpa);
    const int R = nrules[e];
    const unsigned rows = (unsigned)ws.rows[e];
    // uniform exits before staging: the agent is skipped, belongs to the tiled form, or has fewer rows than the workgroups in front hold
    if (rows == 0u || R > resident_rules || (unsigned)wg * (unsigned)(nthr / H) >= rows) return;
    const int RPS = sh.rps;
    const double *rb = rb_all + (size_t)e * (NANT + 1) * maxR;
    double *tab_s = col + (size_t)(NANT + 1) * RPS;
    constexpr bool LT = KIND != FRIRL_HIP_ENV_CARTPOLE;                 // small tables (41-point universes): universes and VE tables in LDS too
    uint32_t *hash_s = reinterpret_cast<uint32_t *>(tab_s + (LT ? 2 * NANT * U : 0));
    const int nj = (R + H - 1) / H;                                    // rules per lane; the padding rules of the last round weigh exactly 0
    resident_stage_image<NANT>(col, RPS, rb, maxR, R, threadIdx.x, nthr);
    for (int i = threadIdx.x; i < NANT * FRIRL_HIP_MAX_GRID; i += nthr) grid_s[i] = ag.grid_values[i];
    if (LT) for (int i = threadIdx.x; i < NANT * U; i += nthr) { tab_s[i] = ve[i]; tab_s[NANT * U + i] = u[i]; }
    for (int i = threadIdx.x; i < sh.ht; i += nthr) hash_s[i] = HT_EMPTY;
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += nthr) hash_insert<NANT>(hash_s, sh.ht, col, RPS, r);
    __syncthreads();                                                   // the last barrier: from here on every wave runs on its own
    const double *ves, *us;
    if constexpr (LT) { ves = tab_s; us = tab_s + NANT * U; } else { ves = ve; us = u; }
    double udiv[NS];                                                   // FIVEInit.c:244-248, once instead of per observation
#pragma unroll
    for (int k = 0; k < NS; k++) udiv[k] = universe_div(us + (size_t)k * U, U);
    auto observe = [&](int k, double x) { const double *uni = us + (size_t)k * U; return ves[(size_t)k * U + snap_index(uni, U, x, udiv[k])]; };

    const int lane = threadIdx.x & (FRIRL_WAVE - 1), h = lane % H;
    const bool leader = (h == 0);
    const auto pk = pin_pow(PowC<NANT>());
    const int cap = ws.cap[e];
    double ave[NA];                                                    // uniform loads: the action VE points stay in scalar registers
#pragma unroll
    for (int a = 0; a < NA; a++) ave[a] = ag.action_ve[a];

    double states[NS], q[NS], cur[NS], total = 0.0, action = 0.0;
    size_t qi = 0;
    int steps = 0, success = 0;
    bool active = false, fresh = false, drained = false;
#pragma unroll
    for (int k = 0; k < NS; k++) { states[k] = 0.0; q[k] = 0.0; cur[k] = 0.0; }

    for (;;) {
        // ---- refill: every idle group takes the agent's next row (one atomic per wave) -------------------------------
        const bool want = !active && !drained;
        const unsigned long long wb = __ballot(want && leader);
        if (wb) {
            const int first = __ffsll((long long)wb) - 1;
            unsigned base = 0u;
            if (lane == first) base = atomicAdd(&ws.next[e], (unsigned)__popcll(wb));
            base = (unsigned)__shfl((int)base, first);
            unsigned item = base + (unsigned)__popcll(wb & ((1ull << lane) - 1ull));
            item = (unsigned)__shfl((int)item, lane - h);
            if (want) {
                if (item < rows) {
                    active = true;
                    success = 0;
                    qi = (size_t)e * ro.n + item;
                    steps = 0;
                    total = 0.0;
#pragma unroll
                    for (int k = 0; k < NS; k++) states[k] = ro.start_states ? ro.start_states[qi * NS + k] : ag.values_def[k];   // frirl_episode.c:46-48
                    fresh = true;
                } else {
                    drained = true;
                }
            }
        }
        if (!__any(active ? 1 : 0)) break;                             // the agent's rows are used up and every episode of this wave has ended

        // ---- the environment's own step (every lane of the group computes the same values) ---------------------------
        if (active) {
            if (fresh) {
#pragma unroll
                for (int k = 0; k < NS; k++) q[k] = observe(k, states[k]);                  // :78 (un-quantised start state)
            } else {
                double r, qs[NS];
                env_do_action(KIND, action, states, cur);                                         // :97
                env_get_reward(KIND, cur, r, success);                                            // :106
                total = total + r;                                                                // :107
                env_quantize(KIND, NS, grid_s, ag.grid_len, ag.grid_div, cur, qs);                // :112
#pragma unroll
                for (int k = 0; k < NS; k++) q[k] = observe(k, qs[k]);
            }
        }

        // ---- frirl_get_best_action (:148): this lane's rules, all actions --------------------------------------------
        double sv[NA], sw[NA];
        unsigned hit[NA];
#pragma unroll
        for (int a = 0; a < NA; a++) { sv[a] = 0.0; sw[a] = 0.0; hit[a] = FRIRL_HIP_NO_HIT; }
        if (active) {
            // exact hits: one table probe per action; a hit's own sums come out of the sweep poisoned (rsq(0)) and are not read
            double key[NANT];
            uint32_t hs = 0u;
#pragma unroll
            for (int k = 0; k < NS; k++) { key[k] = q[k]; hs = hash_mix(hs, q[k]); }
#pragma unroll
            for (int a = 0; a < NA; a++) {
                key[NS] = ave[a];
                hit[a] = hash_lookup<NANT>(hash_s, sh.ht, col, RPS, hs, key);
            }
            resident_sweep<NANT, NA, H, false>(col, nullptr, 0u, q, ave, pk, h, nj, sv, sw);
        }
        if (H > 1) {                                                   // combine the H rule slices (all lanes of the wave take part in the moves)
            group_sum_n<NA>(sv, H);
            group_sum_n<NA>(sw, H);
        }
        if (active) {
            // first maximum in action order, `bv < c` as max.inl:21; action 0 seeds it (a NaN there sticks, as in the reference)
            double bv = 0.0;
            int pa = 0;
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const double c = (hit[a] != FRIRL_HIP_NO_HIT) ? col[(int)hit[a] * (NANT + 1) + NANT] : sv[a] / sw[a];
                if (a == 0 || bv < c) { bv = c; pa = a; }
            }
            bool ended = false;
            if (fresh) {
                pa = e_greedy(ag, pa, (uint32_t)qi, 0u, 0u);
                fresh = false;
            } else {
                pa = e_greedy(ag, pa, (uint32_t)qi, 0u, (uint32_t)(steps + 1));
#pragma unroll
                for (int k = 0; k < NS; k++) states[k] = cur[k];                                         // :163-165
                steps++;                                                                                 // :174
                if (success == 1) ended = true;                                                          // :183
            }
            action = grid_s[NS * FRIRL_HIP_MAX_GRID + pa];                                               // :82 / :151
            if (!ended && steps >= cap) ended = true;                                                    // :86
            if (ended) {
                active = false;
                if (leader) {
                    ro.steps[qi] = steps;
                    ro.reward[qi] = total;
                    if (ro.success) ro.success[qi] = success;
                    if (ro.final_states)
                        for (int k = 0; k < NS; k++) ro.final_states[qi * NS + k] = states[k];
                }
            }
        }
    }
}

// One thread per agent; the rows in order j = 0, 1, ...: the sums do not depend on the lane shape that rolled the rows out.
__global__ __launch_bounds__(256) void rollout_batch_score_kernel(int E, const frirl_hip_rollout_batch_rows ro, frirl_hip_rollout_score *__restrict__ scores)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    frirl_hip_rollout_score s;
    s.rows = 0; s.successes = 0; s.steps_sum = 0; s.reward_sum = 0.0; s.reward_min = 0.0; s.reward_max = 0.0;
    for (int j = 0; j < ro.n; j++) {
        const size_t q = (size_t)e * ro.n + j;
        const int st = ro.steps[q];
        if (st < 0) continue;
        const double r = ro.reward[q];
        s.reward_min = (s.rows == 0 || r < s.reward_min) ? r : s.reward_min;
        s.reward_max = (s.rows == 0 || r > s.reward_max) ? r : s.reward_max;
        s.rows++;
        s.successes += ro.success[q] == 1 ? 1 : 0;
        s.steps_sum += st;
        s.reward_sum = s.reward_sum + r;
    }
    scores[e] = s;
}

}  // namespace frirl

using namespace frirl_host;

namespace {

// control arrays, then the success flags of a call that wants scores but passes no `success`
size_t rollout_batch_layout(char *base, size_t E, size_t n, frirl::RolloutBatchWs *ws, int32_t **success)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    frirl::RolloutBatchWs w;
    w.rows = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.cap = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E));
    w.next = reinterpret_cast<uint32_t *>(take(sizeof(uint32_t) * E));
    int32_t *succ = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * n));
    if (ws) *ws = w;
    if (success) *success = succ;
    return off;
}

template <int N, int NA, int KIND>
size_t resident_lds_bytes(int rps, int ht, int U)
{
    return (size_t)(N + 1) * rps * sizeof(double) + (KIND != FRIRL_HIP_ENV_CARTPOLE ? 2 * sizeof(double) * N * (size_t)U : 0) + sizeof(uint32_t) * (size_t)ht;
}

// Lane-group size and workgroups per agent of the resident form.  A workgroup keeps its agent's image, so what fills the chip is
// workgroups: `slots` of them are resident at once (LDS).  With fewer agents than slots an agent gets several workgroups (each
// stages the image again), and H is the widest group that still gives every row of a workgroup's share its own lanes: 64 for one row
// per agent, 16 for 16 rows, 1 once a workgroup has 256 rows or more to itself.
template <int N, int NA, int KIND, int H>
void launch_resident(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_batch_rows *ro,
                     frirl::ResidentBatchShape sh, int block, int resident_rules, const frirl::RolloutBatchWs &ws, hipStream_t s)
{
    const size_t dyn = resident_lds_bytes<N, NA, KIND>(sh.rps, sh.ht, t->U);
    hipLaunchKernelGGL((frirl::rollout_batch_resident_kernel<N, NA, KIND, H>), dim3((unsigned)b->E * (unsigned)sh.wpa), dim3(block), dyn, s, t->u, t->ve, t->U,
                       b->rb, b->nrules, b->maxR, *ag, sh, resident_rules, *ro, ws);
}

template <int N, int NA, int KIND>
void launch_resident_h(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_batch_rows *ro,
                       int rps, int resident_rules, const frirl::RolloutBatchWs &ws, hipStream_t s)
{
    frirl::ResidentBatchShape sh;
    sh.rps = rps;
    sh.ht = 64;
    while (sh.ht < 2 * rps) sh.ht *= 2;
    const size_t dyn = resident_lds_bytes<N, NA, KIND>(sh.rps, sh.ht, t->U);
    long per_cu = (long)((150 * 1024) / (dyn + 4096));                 // workgroups a CU's LDS holds
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const long slots = per_cu * rb_cus();
    const long n = ro->n;
    long wpa = slots / b->E;
    wpa = wpa < 1 ? 1 : (wpa > n ? n : wpa);
    const long share = (n + wpa - 1) / wpa;                            // rows of a workgroup
    constexpr int HMIN = NA > 8 ? 4 : 1, HMAX = NA > 8 ? 16 : 64;      // the butterfly over 64 lanes would outweigh 3 rules per lane of 21 actions
    int H = HMAX;
    while (H > HMIN && share * H > frirl::RBR_BLOCK) H /= 4;
    const int forced = opts().rollout_batch_slices;
    if ((forced == 1 || forced == 4 || forced == 16 || forced == 64) && forced >= HMIN && forced <= HMAX) H = forced;
    const long wmax = (n * H + frirl::RBR_BLOCK - 1) / frirl::RBR_BLOCK;   // workgroups that n groups of H lanes fill
    wpa = wpa > wmax ? wmax : wpa;
    const long lanes = ((n + wpa - 1) / wpa) * H;
    const int block = lanes >= frirl::RBR_BLOCK ? frirl::RBR_BLOCK : (int)((lanes + FRIRL_WAVE - 1) / FRIRL_WAVE * FRIRL_WAVE);
    sh.wpa = (int)wpa;
#define GO(HH) launch_resident<N, NA, KIND, HH>(t, b, ag, ro, sh, block, resident_rules, ws, s)
    if constexpr (NA > 8) {
        if (H == 16) GO(16); else GO(4);
    } else {
        switch (H) {
            case 1: GO(1); break;
            case 4: GO(4); break;
            case 16: GO(16); break;
            default: GO(64); break;
        }
    }
#undef GO
}

template <int N, int AMAX, int G, int H, bool PN>
void launch_tiled(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_batch_rows *ro, int resident_rules,
                  const frirl::RolloutBatchWs &ws, hipStream_t s)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    const int wpa = (ro->n + EPB - 1) / EPB;
    hipLaunchKernelGGL((frirl::rollout_batch_tiled_kernel<N, AMAX, G, H, PN>), dim3((unsigned)b->E * (unsigned)wpa), dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve, t->U,
                       b->rb, b->nrules, b->maxR, *ag, wpa, resident_rules, *ro, ws);
}

template <int N>
void launch_tiled_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_batch_rows *ro, int resident_rules,
                    const frirl::RolloutBatchWs &ws, hipStream_t s)
{
    frirl::for_batch_shape<N>(ag, rb_rollout_slices(b->E, ro->n, ag->A, 0), [&](auto sh) {
        using S = decltype(sh);
        launch_tiled<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, ro, resident_rules, ws, s);
    });
}

// Rule count up to which an agent of this call is served by the resident form; 0 = the tiled form serves every agent.
int resident_rules_of_call(const frirl_hip_tables *t, const frirl_hip_agent *ag)
{
    const Options &o = opts();
    if (o.rollout_batch_resident == 0) return 0;
    int cap = frirl_hip_rollout_resident_rules(t->nant, ag->A, ag->p, ag->env_kind);     // the demos' shapes, default Shepard power
    if (ag->env_kind != FRIRL_HIP_ENV_CARTPOLE && 2 * sizeof(double) * t->nant * (size_t)t->U > 16 * 1024) cap = 0;   // their tables go to LDS
    if (o.rollout_batch_resident_rules > 0 && o.rollout_batch_resident_rules < cap) cap = o.rollout_batch_resident_rules;
    return cap;
}

}  // namespace

extern "C" size_t frirl_hip_rollout_batch_workspace_bytes(int32_t nant, int32_t E, int32_t maxR, int32_t n, int32_t A)
{
    if (nant < 1 || E < 1 || maxR < 1 || n < 1 || A < 1) return 0;
    return rollout_batch_layout(nullptr, (size_t)E, (size_t)n, nullptr, nullptr);
}

extern "C" int frirl_hip_rollout_batch(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                       const frirl_hip_rollout_batch_rows *ro, frirl_hip_rollout_score *scores, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    static const char *who = "frirl_hip_rollout_batch";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if ((rc = check_rollout_agent_null(agent, ro && ro->steps && ro->reward, who))) return rc;
    if (ro->n < 1) { set_error("%s: n=%d < 1", who, ro->n); return FRIRL_HIP_EINVAL; }
    if ((int64_t)b->E * ro->n > INT32_MAX) { set_error("%s: E * n = %lld rows exceed INT32_MAX", who, (long long)b->E * ro->n); return FRIRL_HIP_EINVAL; }
    if ((rc = check_rollout_agent(t, agent, who))) return rc;
    const size_t E = (size_t)b->E, n = (size_t)ro->n;
    if ((rc = check_workspace(who, workspace, workspace_bytes, rollout_batch_layout(nullptr, E, n, nullptr, nullptr), "frirl_hip_rollout_batch_workspace_bytes")) ||
        (rc = check_device()))
        return rc;
    hipStream_t s = as_stream(stream);
    frirl::RolloutBatchWs ws;
    int32_t *ws_success = nullptr;
    rollout_batch_layout(static_cast<char *>(workspace), E, n, &ws, &ws_success);
    frirl_hip_rollout_batch_rows r = *ro;
    if (scores && !r.success) r.success = ws_success;                  // the scores count successes
    const long Q = (long)E * (long)n;
    hipLaunchKernelGGL(frirl::rollout_batch_prep_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, b->nrules, b->E, b->maxR, agent->max_steps, r, ws);
    const int resident_rules = resident_rules_of_call(t, agent);
    if (resident_rules > 0) {
        const int fit = b->maxR < resident_rules ? b->maxR : resident_rules;
        const int rps = (fit + 63) / 64 * 64;
        if (t->nant == 3) launch_resident_h<3, 3, FRIRL_HIP_ENV_MOUNTAINCAR>(t, b, agent, &r, rps, resident_rules, ws, s);
        else if (agent->A == 3) launch_resident_h<5, 3, FRIRL_HIP_ENV_ACROBOT>(t, b, agent, &r, rps, resident_rules, ws, s);
        else launch_resident_h<5, 21, FRIRL_HIP_ENV_CARTPOLE>(t, b, agent, &r, rps, resident_rules, ws, s);
    }
    if (b->maxR > resident_rules) {                                    // some agent may hold more rules than the resident form takes
        if (t->nant == 3) launch_tiled_n<3>(t, b, agent, &r, resident_rules, ws, s);
        else launch_tiled_n<5>(t, b, agent, &r, resident_rules, ws, s);
    }
    if (scores) hipLaunchKernelGGL(frirl::rollout_batch_score_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, b->E, r, scores);
    return check_launch(who);
}
