// shared.hip -- many observations / environments against ONE read-only rule base (evaluation mode, SURVEY 8f #3, and
// the "try-remove" replays of the rule-base reduction, 8f #1).
//
// Lane = observation (or environment).  A workgroup stages tiles of the rule base in LDS (every rule is fetched from
// HBM/L2 once per workgroup and reused by its 256 lanes), each lane walks the tile's rules in index order and
// accumulates its own Shepard sums sequentially -- the reference's summation order (FIVEVagConcl.c:224-235,
// FIVEVagConcl_FRIRL_BestAct.c:212-217) -- so no reductions are needed.  Compute-bound: ~24 FP64 instructions per
// (lane, rule, action).
#include "rollout_episode.h"
#include "reduce_plan.h"
#include "shape_ladder.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <numeric>
#include <vector>

namespace frirl {

template <int NANT, int AMAX, bool GBA>
__global__ __launch_bounds__(SH_BLOCK) void shared_q_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                             const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR, int p,
                                                             int Q, const double *__restrict__ x, const double *__restrict__ action_ve, int A,
                                                             double *__restrict__ conc, uint32_t *__restrict__ hit, int32_t *__restrict__ best)
{
    constexpr int ND = GBA ? NANT - 1 : NANT;    // observation dimensions supplied by the caller
    __shared__ SharedTile<NANT> tl;
    const int qi = blockIdx.x * SH_BLOCK + threadIdx.x;
    const bool live = qi < Q;
    double q[ND];
#pragma unroll
    for (int k = 0; k < ND; k++) q[k] = live ? observe_ve(u, ve, U, k, x[(size_t)qi * ND + k]) : 0.0;
    if (GBA && (int)threadIdx.x < A) tl.ave[threadIdx.x] = action_ve[threadIdx.x];
    unsigned h0;
    int bi;
    double bv;
    shared_sweep<NANT, AMAX, GBA, false>(tl, rb, nullptr, nrules[0], maxR, PowU{p}, 0, A, GBA ? (A + AMAX - 1) / AMAX : 1, q, live, 0u,
                                         live ? conc + (size_t)qi * (GBA ? A : 1) : nullptr, h0, bi, bv);
    if (!live) return;
    if (GBA) best[qi] = bi;
    else hit[qi] = h0;
}

// frirl_test_run's episode (src/frirl/frirl_test_run.c:66-70: construct_rb = 0, reduction_state = 1, frirl_episode) for
// Q environments sharing one rule base, the whole roll-out in one launch.  No SARSA update (frirl_episode.c:155), so the
// rule base stays read-only and can be shared.  G consecutive lanes serve one environment, each evaluating its own
// block of actions (G = 1 for throughput when Q fills the chip; G = 4 / 8 cut the per-step latency when Q is small, the
// case of the reduction's replays); the environment state is kept redundantly by all G lanes.
// PN: Shepard power = the default nant as a compile-time constant; else the agent's run-time power (instantiated without rule slices)
template <int NANT, int AMAX, int G, int H, bool EXCL, bool PN = true>
__global__ __launch_bounds__(SH_BLOCK) void rollout_shared_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                   const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                   const frirl_hip_agent ag, int Q, const frirl_hip_rollout ro,
                                                                   const unsigned *__restrict__ run_if)
{
    constexpr int NS = NANT - 1, GH = G * H, EPB = SH_BLOCK / GH;
    if (run_if && *run_if == 0u) return;          // the resident form (rollout.hip) has served this call
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int gl = threadIdx.x % GH;
    const int qi = blockIdx.x * EPB + threadIdx.x / GH;
    const bool exists = qi < Q;
    const int R = nrules[0];
    using POW = typename std::conditional<PN, PowC<NANT>, PowU>::type;
    POW p;
    if constexpr (!PN) p.p = ag.p > 0 ? ag.p : NANT;
    const uint32_t mask = (EXCL && exists && ro.exclude_mask) ? ro.exclude_mask[qi] : 0u;
    double states[NS], total;
    int steps, success;
    rollout_episode<NANT, AMAX, G, H, EXCL, POW>(tl, grid_s, u, ve, U, rb, ro.rule_slot, R, maxR, ag, p, exists, (uint32_t)qi, mask,
                                                  ro.start_states ? ro.start_states + (size_t)(exists ? qi : 0) * NS : nullptr, ag.max_steps, steps,
                                                  total, success, states);
    if (!exists || gl != 0) return;
    ro.steps[qi] = steps;
    ro.reward[qi] = total;
    if (ro.success) ro.success[qi] = success;
    if (ro.final_states)
        for (int k = 0; k < NS; k++) ro.final_states[(size_t)qi * NS + k] = states[k];
}

}  // namespace frirl

using namespace frirl_host;

static int check_shared_args(const frirl_hip_tables *t, const frirl_hip_rulebases *b, int Q, const char *who)
{
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (b->E != 1) { set_error("%s: needs ONE shared rule base (E == 1), got E=%d", who, b->E); return FRIRL_HIP_EINVAL; }
    if (Q < 1) { set_error("%s: Q=%d < 1", who, Q); return FRIRL_HIP_EINVAL; }
    if (t->nant < 2 || t->nant > 9) { set_error("%s: nant=%d outside 2..9", who, t->nant); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

static int check_shared(const frirl_hip_tables *t, const frirl_hip_rulebases *b, int Q, const char *who)
{
    int rc = check_shared_args(t, b, Q, who);
    return rc ? rc : check_device();
}

int frirl_host::check_grid_len(const frirl_hip_tables *t, const frirl_hip_agent *a, const char *who)
{
    for (int k = 0; k < t->nant; k++)
        if (a->grid_len[k] < 1 || a->grid_len[k] > FRIRL_HIP_MAX_GRID) { set_error("%s: grid_len[%d]=%d outside 1..%d", who, k, a->grid_len[k], FRIRL_HIP_MAX_GRID); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

// the roll-outs run the demo dynamics on the device: env_kind must name one of them, with its antecedent count
int frirl_host::check_demo_kind(const frirl_hip_tables *t, const frirl_hip_agent *agent, const char *who)
{
    if (agent->env_kind < 0 || agent->env_kind > 2 || (agent->env_kind == FRIRL_HIP_ENV_MOUNTAINCAR ? t->nant != 3 : t->nant != 5)) {
        set_error("%s: env_kind %d does not match nant=%d (the demo environments only)", who, agent->env_kind, t->nant);
        return FRIRL_HIP_EINVAL;
    }
    return FRIRL_HIP_OK;
}

extern "C" int five_hip_vag_concl_shared(const frirl_hip_tables *t, const frirl_hip_rulebases *b, int p, int32_t Q, const double *x,
                                         double *conc, uint32_t *hit, void *stream)
{
    int rc = check_shared(t, b, Q, "five_hip_vag_concl_shared");
    if (rc) return rc;
    if (!x || !conc || !hit) { set_error("five_hip_vag_concl_shared: NULL argument"); return FRIRL_HIP_EINVAL; }
    const int pp = p > 0 ? p : t->nant;
    const dim3 grid((Q + frirl::SH_BLOCK - 1) / frirl::SH_BLOCK);
    switch (t->nant) {
#define M(N) case N: hipLaunchKernelGGL((frirl::shared_q_kernel<N, 1, false>), grid, dim3(frirl::SH_BLOCK), 0, as_stream(stream), t->u, t->ve, t->U, b->rb, \
                                        b->nrules, b->maxR, pp, Q, x, nullptr, 1, conc, hit, nullptr); break;
        M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9)
#undef M
    }
    return check_launch("five_hip_vag_concl_shared");
}

extern "C" int frirl_hip_get_best_action_shared(const frirl_hip_tables *t, const frirl_hip_rulebases *b, int p, int32_t Q, const double *states,
                                                const double *action_ve, int A, double *actconc, int32_t *best, void *stream)
{
    int rc = check_shared(t, b, Q, "frirl_hip_get_best_action_shared");
    if (rc) return rc;
    if (!states || !action_ve || !actconc || !best || A < 1 || A > FRIRL_HIP_MAX_ACTIONS) { set_error("frirl_hip_get_best_action_shared: bad arguments"); return FRIRL_HIP_EINVAL; }
    const int pp = p > 0 ? p : t->nant;
    const dim3 grid((Q + frirl::SH_BLOCK - 1) / frirl::SH_BLOCK);
    switch (t->nant) {
#define M(N)                                                                                                                                              \
    case N:                                                                                                                                               \
        if (A <= 4) hipLaunchKernelGGL((frirl::shared_q_kernel<N, 4, true>), grid, dim3(frirl::SH_BLOCK), 0, as_stream(stream), t->u, t->ve, t->U, b->rb,   \
                                       b->nrules, b->maxR, pp, Q, states, action_ve, A, actconc, nullptr, best);                                          \
        else hipLaunchKernelGGL((frirl::shared_q_kernel<N, 8, true>), grid, dim3(frirl::SH_BLOCK), 0, as_stream(stream), t->u, t->ve, t->U, b->rb,         \
                                b->nrules, b->maxR, pp, Q, states, action_ve, A, actconc, nullptr, best);                                                 \
        break;
        M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9)
#undef M
    }
    return check_launch("frirl_hip_get_best_action_shared");
}

template <int N, int AMAX, int G, int H, bool PN = true>
static void launch_rollout(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, int Q, const frirl_hip_rollout *ro,
                           hipStream_t s, const unsigned *run_if)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    const dim3 grid((Q + EPB - 1) / EPB);
    if (ro->exclude_mask && ro->rule_slot)
        hipLaunchKernelGGL((frirl::rollout_shared_kernel<N, AMAX, G, H, true, PN>), grid, dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, Q, *ro, run_if);
    else
        hipLaunchKernelGGL((frirl::rollout_shared_kernel<N, AMAX, G, H, false, PN>), grid, dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules, b->maxR, *ag, Q, *ro, run_if);
}

// lanes per environment and rule slices: lane_group / lane_slices; the compiled variant: for_shared_shape (shape_ladder.h)
template <int N>
static void launch_rollout_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, int Q, const frirl_hip_rollout *ro,
                             hipStream_t s, const unsigned *run_if)
{
    const int G = lane_group(opts().rollout_group, Q, ag->A), H = lane_slices(opts().rollout_slices, Q, G);
    frirl::for_shared_shape<N>(ag, G, H, [&](auto sh) {
        using S = decltype(sh);
        launch_rollout<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, Q, ro, s, run_if);
    });
}

int frirl_rollout_resident(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, int Q, const frirl_hip_rollout *ro,
                           hipStream_t s, const unsigned **too_big_flag, void **workspace);      // rollout.hip

extern "C" int frirl_hip_rollout_shared(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, int32_t Q,
                                        const frirl_hip_rollout *ro, void *stream)
{
    int rc = check_shared_args(t, b, Q, "frirl_hip_rollout_shared");
    if (rc) return rc;
    if (!agent || !ro || !ro->steps || !ro->reward || !agent->grid_values || !agent->action_ve) { set_error("frirl_hip_rollout_shared: NULL argument"); return FRIRL_HIP_EINVAL; }
    if (agent->A < 1 || agent->A > FRIRL_HIP_MAX_ACTIONS || agent->max_steps < 0) { set_error("frirl_hip_rollout_shared: A=%d / max_steps=%d out of range", agent->A, agent->max_steps); return FRIRL_HIP_EINVAL; }
    if ((rc = check_grid_len(t, agent, "frirl_hip_rollout_shared"))) return rc;
    if ((ro->exclude_mask == nullptr) != (ro->rule_slot == nullptr)) { set_error("frirl_hip_rollout_shared: exclude_mask and rule_slot go together"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, "frirl_hip_rollout_shared")) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    // small rule bases: the LDS-resident, queue-fed form (rollout.hip); the tiled kernel below serves every other shape, and a rule
    // base that turns out not to fit the LDS image (known on the device only: `too_big`)
    const unsigned *too_big = nullptr;
    void *ws = nullptr;
    if (frirl_rollout_resident(t, b, agent, Q, ro, s, &too_big, &ws)) {
        if (too_big) {
            if (t->nant == 3) launch_rollout_n<3>(t, b, agent, Q, ro, s, too_big);
            else launch_rollout_n<5>(t, b, agent, Q, ro, s, too_big);
        }
        if (ws) (void)hipFreeAsync(ws, s);
        return check_launch("frirl_hip_rollout_shared");
    }
    if (t->nant == 3) launch_rollout_n<3>(t, b, agent, Q, ro, s, nullptr);
    else launch_rollout_n<5>(t, b, agent, Q, ro, s, nullptr);
    return check_launch("frirl_hip_rollout_shared");
}

// ---- speculative try-remove reduction (frirl_sequential_run.c:170-350); see include/frirl_hip.h ----------------------
namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess; }
};
}  // namespace

extern "C" int frirl_hip_reduce_shared(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant, int strategy,
                                       double reward_tolerance, int depth, int32_t *kept, frirl_hip_reduce_result *result, void *stream)
{
    int rc = check_shared_args(t, b, 1, "frirl_hip_reduce_shared");
    if (rc) return rc;
    if (!agent || !result) { set_error("frirl_hip_reduce_shared: NULL argument"); return FRIRL_HIP_EINVAL; }
    if (strategy != 1 && strategy != 2) { set_error("frirl_hip_reduce_shared: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", strategy); return FRIRL_HIP_EINVAL; }
    if (depth == 0) depth = 10;
    if (depth < 1 || depth > frirl::RW_MAX_DEPTH) { set_error("frirl_hip_reduce_shared: depth %d outside 1..%d", depth, frirl::RW_MAX_DEPTH); return FRIRL_HIP_EINVAL; }
    if ((rc = check_demo_kind(t, agent, "frirl_hip_reduce_shared")) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    // candidate order, mask tables, tree walk and compaction: reduce_plan.h (shared with the caller-stepped form, policy.hip)
    ReducePlan plan;
    if ((rc = plan.load("frirl_hip_reduce_shared", t, b, rant, strategy, depth, s))) return rc;
    const int lanes_max = plan.lanes_max();
    DevBuf d_slot, d_mask, d_steps, d_reward;
    if (!d_slot.alloc((size_t)b->maxR) || !d_mask.alloc(sizeof(uint32_t) * lanes_max) || !d_steps.alloc(sizeof(int32_t) * lanes_max) ||
        !d_reward.alloc(sizeof(double) * lanes_max)) { set_error("frirl_hip_reduce_shared: hipMalloc failed"); return FRIRL_HIP_ELAUNCH; }
    std::vector<int32_t> steps(lanes_max);
    std::vector<double> reward(lanes_max);

    // baseline replay on the un-reduced rule base (:196-198 and the first loop iteration, :204-206)
    frirl_hip_rollout ro = {};
    ro.steps = static_cast<int32_t *>(d_steps.p);
    ro.reward = static_cast<double *>(d_reward.p);
    frirl_hip_agent greedy = *agent;
    greedy.no_random = 1;                                             // the replays are greedy (reduction_state == 1 keeps epsilon at 0 in every demo)
    rc = frirl_hip_rollout_shared(t, b, &greedy, 1, &ro, stream);
    if (rc) return rc;
    FRIRL_HIP_TRY(hipMemcpyAsync(steps.data(), d_steps.p, sizeof(int32_t), hipMemcpyDeviceToHost, s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipMemcpyAsync(reward.data(), d_reward.p, sizeof(double), hipMemcpyDeviceToHost, s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
    plan.set_baseline(steps[0], reward[0]);
    frirl_hip_agent capped = greedy;
    capped.max_steps = plan.capped_steps(capped.max_steps);

    ro.exclude_mask = static_cast<const uint32_t *>(d_mask.p);
    ro.rule_slot = static_cast<const uint8_t *>(d_slot.p);
    for (;;) {
        int lanes = 0;
        if ((rc = plan.open_round(d_slot.p, d_mask.p, s, &lanes))) return rc;
        if (lanes == 0) break;
        rc = frirl_hip_rollout_shared(t, b, &capped, lanes, &ro, stream);
        if (rc) return rc;
        FRIRL_HIP_TRY(hipMemcpyAsync(steps.data(), d_steps.p, sizeof(int32_t) * lanes, hipMemcpyDeviceToHost, s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
        FRIRL_HIP_TRY(hipMemcpyAsync(reward.data(), d_reward.p, sizeof(double) * lanes, hipMemcpyDeviceToHost, s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
        FRIRL_HIP_TRY(hipStreamSynchronize(s), "frirl_hip_reduce_shared", return FRIRL_HIP_ELAUNCH);
        if ((rc = plan.close_round(steps.data(), reward.data(), agent->reward_good_above, reward_tolerance, s))) return rc;
    }
    plan.result(kept, result);
    return FRIRL_HIP_OK;
}
