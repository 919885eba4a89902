// episode_kernel.h -- the fused episode kernels (frirl_episode's begin and step) and their launchers.
//
// Shared by sarsa.hip (the demo environments: the dynamics run on the device, picked by agent.env_kind) and agent_i<N>.hip
// (EXT = true: the caller steps its own environment and hands the observation, reward and success flag to
// frirl_hip_agent_observe; one translation unit per antecedent count so the build compiles them in parallel).  With EXT =
// false the kernels are the demo kernels: the caller's-data argument (ext_io.h; agent.hip packs it once per call) is an empty struct
// and every EXT branch is compiled out.
#pragma once

#include "envs.h"
#include "ext_io.h"
#include "sweeps.h"

namespace frirl {

// imitation (reference frirl_episode.c:58-79,127-151: keyaction replaces the epsilon-greedy action; key 32 = the agent chooses): row e
// takes teacher[e] when it is an action index, and keeps `chosen` for any other value.  The exploration stream is counter-based, so
// a taught pick consumes nothing of it.
__device__ __forceinline__ int taught_action(const ExtIo &io, int e, int A, int chosen)
{
    if (!io.teacher) return chosen;
    const int32_t k = io.teacher[e];
    return (k >= 0 && k < A) ? k : chosen;
}

// The learning hyper-parameters the step reads (frirl_update_sarsa.c:358,363, update_rules :30-126), under the field names of
// frirl_hip_agent: the demo kernels read them from the launch's agent itself; the EXT kernels build the workgroup's own copy, row e
// of every column of io.rows that is given.  One workgroup serves one row, so the values are wave-uniform: they are moved to scalar
// registers, where the launch's own live (as vector registers they cost some variants a wave per SIMD).
// `epsilon` is the row's exploration rate in the episode whose stream key is `key` (frirl_hip_explore_rows, envs.h: explore_epsilon).
struct StepHparams {
    double alpha, gamma, qdiff_pos_boundary, qdiff_neg_boundary, weight_significant, epsilon;
    int32_t skip_rules;
};
__device__ __forceinline__ double explore_rate(const frirl_hip_agent &ag, const ExtIo &io, int e, uint32_t key)
{
    const double eps = io.ex.epsilon ? io.ex.epsilon[e] : ag.epsilon;
    const int32_t h = io.ex.horizon ? io.ex.horizon[e] : io.ex.horizon_all;
    return explore_epsilon(eps, h, key);
}
__device__ __forceinline__ const frirl_hip_agent &step_hparams(const frirl_hip_agent &ag, const NoIo &, const frirl_hip_envs &, int) { return ag; }
__device__ __forceinline__ StepHparams step_hparams(const frirl_hip_agent &ag, const ExtIo &io, const frirl_hip_envs &ev, int e)
{
    const frirl_hip_hparam_rows &r = io.rows;
    StepHparams h;
    h.alpha = r.alpha ? wave_uniform(r.alpha[e]) : ag.alpha;
    h.gamma = r.gamma ? wave_uniform(r.gamma[e]) : ag.gamma;
    h.qdiff_pos_boundary = r.qdiff_pos_boundary ? wave_uniform(r.qdiff_pos_boundary[e]) : ag.qdiff_pos_boundary;
    h.qdiff_neg_boundary = r.qdiff_neg_boundary ? wave_uniform(r.qdiff_neg_boundary[e]) : ag.qdiff_neg_boundary;
    h.weight_significant = r.weight_significant ? wave_uniform(r.weight_significant[e]) : ag.weight_significant;
    h.skip_rules = r.skip_rules ? __builtin_amdgcn_readfirstlane(r.skip_rules[e]) : ag.skip_rules;
    h.epsilon = wave_uniform(explore_rate(ag, io, e, ev.episode ? (uint32_t)ev.episode[e] : 0u));
    return h;
}

struct StepShared {
    double q_ant[FRIRL_HIP_MAX_NANT];      // raw antecedent values of (s, a)
    double cur_q_ant[FRIRL_HIP_MAX_NANT];  // raw antecedent values of (s', a')
    double ve1[FRIRL_HIP_MAX_NANT];        // VE values of q_ant
    double ve2[FRIRL_HIP_MAX_NANT];        // VE values of cur_q_ant
    double rant[FRIRL_HIP_MAX_NANT];       // grid-snapped antecedents of a would-be new rule
    double ve3[FRIRL_HIP_MAX_NANT];        // their VE values
    double cur_states[FRIRL_HIP_MAX_NANT];
    unsigned idx3[FRIRL_HIP_MAX_NANT];    // universe indices of the snapped antecedents
    double reward;
    int success;
    int same;
};

// test hook: frirl_hip_agent.debug_flags bit 0 forces update_rules' second sweep (the candidate path must give the same bits)
__device__ __forceinline__ bool frirl_no_spread_candidates(const frirl_hip_agent &ag) { return (ag.debug_flags & 1) != 0; }

// frirl_update_sarsa + update_rules (reference src/frirl/frirl_update_sarsa.c:348-385, :22-143).
// `qp_known`: Q(s',a') already available (fused step: the greedy sweep produced it, identical
// operands and order -- SURVEY 7(i)); otherwise it is computed by a sweep over ve2.  `hp`: the six learning hyper-parameters, `ag` itself
// or a StepHparams (of `ag` only the grids and the debug flags are read).
template <int NANT, int BLOCK, bool TRACK = false, class COLS, class POW, class HP>
__device__ int update_sarsa_block_hp(const COLS &cols, const double *__restrict__ u, const double *__restrict__ ve, int U, double *__restrict__ base,
                                     int maxR, int32_t *nrules_e, const frirl_hip_agent &ag, const HP &hp, StepShared &sh, double reward,
                                     bool qp_known, double qp, int32_t *fus_e, double *rant_e, BlockRed<BLOCK> &red,
                                     const QResult *rn_known, uint16_t *uidx_e, POW p, SpreadCand *slot, double *spread_ant_e, int32_t *spread_R_e)
{
    const int R = *nrules_e;
    double q1[NANT], q2[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) { q1[k] = sh.ve1[k]; q2[k] = sh.ve2[k]; }
    double *qcol = base + (size_t)NANT * maxR;

    if (!qp_known) {                                                        // :356  Q(s',a')
        const QResult rp = sweep_q<NANT, BLOCK>(cols, qcol, R, q2, p, red);
        qp = (rp.hit != FRIRL_HIP_NO_HIT) ? qcol[rp.hit] : rp.vagc / rp.ws;
    }
    const QResult rn = rn_known ? *rn_known : sweep_q<NANT, BLOCK, TRACK>(cols, qcol, R, q1, p, red, hp.weight_significant, slot);    // :357  Q(s,a)
    const double qnow = (rn.hit != FRIRL_HIP_NO_HIT) ? qcol[rn.hit] : rn.vagc / rn.ws;
    const double qdiff = hp.alpha * (reward + hp.gamma * qp - qnow);        // :358
    int fus = *fus_e;
    __syncthreads();   // every thread has read *fus_e / *nrules_e before thread 0 may rewrite them

    if (qdiff > hp.qdiff_pos_boundary || qdiff < hp.qdiff_neg_boundary) {   // :363
        // snap the antecedents to the allowed grid (check_possible_states, :146-170)
        if (threadIdx.x < NANT) {
            const int k = threadIdx.x;
            const double r = check_possible_states(sh.q_ant[k], ag.grid_values + (size_t)k * FRIRL_HIP_MAX_GRID, ag.grid_len[k]);
            sh.rant[k] = r;
            const double *uni = u + (size_t)k * U;
            const unsigned j = snap_index(uni, U, r, universe_div(uni, U));
            sh.idx3[k] = j;
            sh.ve3[k] = ve[(size_t)k * U + j];
        }
        __syncthreads();
        double q3[NANT];
        bool same = true;
#pragma unroll
        for (int k = 0; k < NANT; k++) { q3[k] = sh.ve3[k]; same = same && (q3[k] == q1[k]); }
        QResult rr = rn;                                                    // :370 (same VE point => same sweep result)
        if (!same) rr = sweep_q<NANT, BLOCK>(cols, qcol, R, q3, p, red);
        if (rr.hit == FRIRL_HIP_NO_HIT) {                                   // :373-377 append and leave
            if (R >= maxR) return FRIRL_HIP_UPD_FULL;
            const double rconc = rr.vagc / rr.ws;
            if (threadIdx.x < NANT) {
                base[(size_t)threadIdx.x * maxR + R] = q3[threadIdx.x];      // five_add_rule.c:80-81
                if (uidx_e) uidx_e[(size_t)threadIdx.x * maxR + R] = (uint16_t)sh.idx3[threadIdx.x];   // five_add_rule.c:76
                if (rant_e) rant_e[(size_t)threadIdx.x * maxR + R] = sh.rant[threadIdx.x];
            }
            if (threadIdx.x == 0) {
                qcol[R] = rconc + qdiff;
                *nrules_e = R + 1;
                *fus_e = 1;
            }
            return FRIRL_HIP_UPD_INSERTED;
        }
        fus = 0;                                                            // :378
    }

    // update_rules (:22-143); FIVE_vag_concl_weight(q_ant) sees the distances of the sweep above
    int rules = R;
    if (fus) rules--;                                                       // :30-33
    int status;
    if (rn.hit != FRIRL_HIP_NO_HIT && (hp.skip_rules == 0 || (hp.skip_rules == 1 && (int)rn.hit < rules))) {
        if (threadIdx.x == 0) qcol[rn.hit] = qnow + qdiff;                  // :55
        status = FRIRL_HIP_UPD_EXACT;
    } else if (hp.skip_rules == 1 && rn.hit != FRIRL_HIP_NO_HIT && (int)rn.hit == rules) {
        status = FRIRL_HIP_UPD_SKIPPED;                                     // :61-63
    } else {
        if (hp.skip_rules == 0) fus = 0;                                    // :70-73
        const int r_skip = fus ? R - 1 : -1;                                // :76,124-126: the just-inserted rule keeps its Q
        if (rn.hit == FRIRL_HIP_NO_HIT) {      // FIVE_vag_concl_weight interpolated (:40): this call defines FIVERB.weights from now on
            if (spread_ant_e && threadIdx.x < NANT) spread_ant_e[threadIdx.x] = sh.q_ant[threadIdx.x];
            if (spread_R_e && threadIdx.x == 0) *spread_R_e = R;
        }
        // K6+K7: from the candidates tracked during the Q(s,a) sweep when possible (no second pass over the slab), else the sweep
        const bool from_cand = TRACK && rn.tracked && rn.hit == FRIRL_HIP_NO_HIT && !frirl_no_spread_candidates(ag) &&
                               spread_from_candidates<BLOCK>(slot[threadIdx.x], qcol, rn.ws, qnow, qdiff, hp.weight_significant, r_skip, red);
        if (!from_cand) sweep_update<NANT, BLOCK>(cols, qcol, R, q1, p, rn.ws, qnow, qdiff, hp.weight_significant, r_skip);
        status = FRIRL_HIP_UPD_SPREAD;
    }
    if (threadIdx.x == 0) *fus_e = fus;
    return status;
}

// ... with the launch's own hyper-parameters (every caller but the EXT step kernel, which passes row e of frirl_hip_hparam_rows)
template <int NANT, int BLOCK, bool TRACK = false, class COLS, class POW>
__device__ __forceinline__ int update_sarsa_block(const COLS &cols, const double *__restrict__ u, const double *__restrict__ ve, int U, double *__restrict__ base,
                                                  int maxR, int32_t *nrules_e, const frirl_hip_agent &ag, StepShared &sh, double reward,
                                                  bool qp_known, double qp, int32_t *fus_e, double *rant_e, BlockRed<BLOCK> &red,
                                                  const QResult *rn_known, uint16_t *uidx_e, POW p, SpreadCand *slot, double *spread_ant_e = nullptr, int32_t *spread_R_e = nullptr)
{
    return update_sarsa_block_hp<NANT, BLOCK, TRACK>(cols, u, ve, U, base, maxR, nrules_e, ag, ag, sh, reward, qp_known, qp, fus_e, rant_e, red, rn_known, uidx_e, p,
                                                     slot, spread_ant_e, spread_R_e);
}

// frirl_episode(): start of an episode (reference src/frirl/frirl_episode.c:46-82).
// EXT: the start state is the caller's observation io.obs (un-quantised, :46-48), and only rows with io.reset[e] != 0 (or
// every row when io.reset is NULL) start an episode; the first action is also written to io.action_out / io.action_idx.
template <int NANT, int AMAX, int BLOCK, bool IDX, bool PN, bool EXT = false>
__global__ __launch_bounds__(BLOCK) void episode_begin_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                               const double *__restrict__ rb, const uint16_t *__restrict__ uidx,
                                                               const int32_t *__restrict__ nrules,
                                                               int maxR, const frirl_hip_agent ag, const frirl_hip_envs ev, const IoArg<EXT> io)
{
    constexpr int NS = NANT - 1;
    const int e = blockIdx.x;
    if constexpr (EXT) {
        if (io.reset && !io.reset[e]) return;           // workgroup-uniform: the row keeps its episode
    }
    extern __shared__ double tab_s[];
    __shared__ double q_s[NS];
    __shared__ GbaScratch<AMAX, BLOCK> gs;
    if (IDX) for (int i = threadIdx.x; i < NANT * U; i += BLOCK) tab_s[i] = ve[i];
    if (threadIdx.x < NS) {
        double v;
        if constexpr (EXT) v = io.obs[(size_t)e * NS + threadIdx.x];                                                        // the caller's start state
        else v = ev.start_states ? ev.start_states[(size_t)e * NS + threadIdx.x] : ag.values_def[threadIdx.x];   // q_states = states = values_def (:46-48)
        ev.states[(size_t)e * NS + threadIdx.x] = v;
        ev.q_ant[(size_t)e * NANT + threadIdx.x] = v;
        q_s[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, v);
    }
    if ((int)threadIdx.x < ag.A) gs.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
    __syncthreads();
    double q[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) q[k] = q_s[k];
    const double *base = rb + (size_t)e * (NANT + 1) * maxR;
    const double *qcol = base + (size_t)NANT * maxR;
    const auto cols = ColsSel<IDX>::make(base, uidx + (IDX ? (size_t)e * NANT * maxR : 0), tab_s, maxR, U);
    const auto pw = PowSel<PN, NANT>::make(ag.p > 0 ? ag.p : NANT);
    int a0;
    if constexpr (AMAX == 24) {
        __shared__ BlockRed<BLOCK> red;
        double dummy[NANT] = {};
        a0 = sweep_gba_many<NANT, AMAX, BLOCK, false>(cols, qcol, nrules[e], q, dummy, pw, ag.A, gs, red, nullptr);   // :78
    } else if constexpr (AMAX > 8) {
        __shared__ BlockRed<BLOCK> red;
        double dummy[NANT] = {};
        a0 = sweep_gba_wide<NANT, 8, AMAX, BLOCK, false>(cols, qcol, nrules[e], q, dummy, pw, ag.A, gs, red, nullptr);   // :78
    } else {
        a0 = sweep_gba<NANT, AMAX, BLOCK>(cols, qcol, nrules[e], q, pw, ag.A, gs);   // :78
    }
    if (threadIdx.x == 0) {
        const uint32_t epi = ev.episode ? (uint32_t)(ev.episode[e] + 1) : 0u;
        if (ev.episode) ev.episode[e] = (int32_t)epi;
        if constexpr (EXT) a0 = e_greedy(ag, explore_rate(ag, io, e, epi), a0, (uint32_t)e, epi, 0u);        // the rate of the episode that starts
        else a0 = e_greedy(ag, a0, (uint32_t)e, epi, 0u);
        if constexpr (EXT) a0 = taught_action(io, e, ag.A, a0);                                                    // :58-79
        ev.q_ant[(size_t)e * NANT + NS] = ag.grid_values[(size_t)NS * FRIRL_HIP_MAX_GRID + a0];                 // :82
        if constexpr (EXT) {
            io.action_out[e] = ag.grid_values[(size_t)NS * FRIRL_HIP_MAX_GRID + a0];
            if (io.action_idx) io.action_idx[e] = a0;
        }
        ev.done[e] = 0;
        ev.ep_steps[e] = 0;
        ev.ep_reward[e] = 0.0;
        if (ev.status) ev.status[e] = FRIRL_HIP_UPD_INACTIVE;
    }
}

// frirl_episode(): one step of the loop (reference src/frirl/frirl_episode.c:86-185), fused.
// register budget of the step kernel: 6 waves per SIMD (<= 80 VGPRs) for the 3-antecedent / <= 4-action shape (it needs ~64 now that
// the observations sit in SGPRs and exact hits need no registers; 8 waves -- all 8192 one-wave environments of the 8192 x 8192 shape
// resident at once -- measured the same 0.24 ms: the kernel is issue-bound, profiles/r02_step_timeline.txt), 4 (<= 128) for the
// others: without the bound the 5-antecedent, many-action variants sit just above 128 and lose a wave
// (the action-parallel kernel, amax > 8: 3 waves = 168 VGPRs -- its branch-free conclusion terms keep more chains in flight, and with
// cartpole's 40 KB of LDS tables only three workgroups fit a CU anyway)
#ifndef FRIRL_STEP_WAVES_N3
#define FRIRL_STEP_WAVES_N3 6
#endif
#ifndef FRIRL_STEP_SAME_CELL
#define FRIRL_STEP_SAME_CELL 1     // 0: always the full pending distance (A/B builds)
#endif
constexpr int step_min_waves(int nant, int amax) { return (nant <= 3 && amax <= 4) ? FRIRL_STEP_WAVES_N3 : (amax > 8 ? 3 : 4); }

// TRACK: the candidates of update_rules' write-back are collected during the fused sweep (sweeps.h: SpreadCand) -- for LARGE rule
// bases, where the second sweep it saves is a second pass over HBM; small slabs are re-read from L2 and the plain form is faster.
#ifdef FRIRL_STEP_TIMING
// experiment build only (tools/build_variant.sh timing -DFRIRL_STEP_TIMING): when each workgroup of the step kernel started, finished its
// fused sweep and left, in 10 ns ticks of the device wall clock -- read back with frirl_hip_debug_step_timing
static __device__ long long g_step_timing[4 * 65536];
#endif

// EXT (frirl_hip_agent_observe): do_action / get_reward / quantize_observations are the caller's -- thread 0 reads the new
// observation, reward and success flag from `io` and quantises with io.q_obs, or with the generic grid rule when that is NULL;
// everything after that is the demo step.  The chosen action is also written to io.action_out / io.action_idx.
template <int NANT, int AMAX, int BLOCK, bool IDX, bool PN, bool TRACK, bool EXT = false>
__global__ __launch_bounds__(BLOCK, step_min_waves(NANT, AMAX)) void episode_step_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                              double *__restrict__ rb, uint16_t *__restrict__ uidx, int32_t *__restrict__ nrules,
                                                              int maxR, const frirl_hip_agent ag, const frirl_hip_envs ev, const IoArg<EXT> io)
{
    constexpr int NS = NANT - 1;
    const int e = blockIdx.x;
#ifdef FRIRL_STEP_TIMING
    static_assert(!EXT, "step timing: demo kernels only");
    const long long tm0 = wall_clock64();
#endif
    if (ev.done[e]) {
        if (threadIdx.x == 0 && ev.status) ev.status[e] = FRIRL_HIP_UPD_INACTIVE;
        return;
    }
    decltype(auto) hp = step_hparams(ag, io, ev, e);         // `ag` itself; EXT: its own copy, row e of the columns of io.rows that are given
    extern __shared__ double tab_s[];
    __shared__ StepShared sh;
    __shared__ BlockRed<BLOCK> red;
    __shared__ GbaScratch<AMAX, BLOCK> gs;
    __shared__ SpreadCand cand_s[TRACK ? BLOCK : 1];       // one slot per lane: candidates of update_rules' write-back (sweeps.h)
    __shared__ double qp_s;                                // EXT: what the update learns towards, formed by thread 0 at the pick
    if (IDX) for (int i = threadIdx.x; i < NANT * U; i += BLOCK) tab_s[i] = ve[i];
    if (threadIdx.x == 0) {
        double s[FRIRL_HIP_MAX_NANT], q[FRIRL_HIP_MAX_NANT];
        if constexpr (EXT) {
            (void)s;
            for (int i = 0; i < NANT; i++) sh.q_ant[i] = ev.q_ant[(size_t)e * NANT + i];
            for (int i = 0; i < NS; i++) sh.cur_states[i] = io.obs[(size_t)e * NS + i];                // the caller's do_action (:97)
            sh.reward = io.reward[e];                                                                 // ... and get_reward (:106)
            sh.success = io.success[e];
            if (io.q_obs) for (int i = 0; i < NS; i++) q[i] = io.q_obs[(size_t)e * NS + i];          // its own quantize_observations (:112)
            else env_quantize(FRIRL_HIP_ENV_EXTERNAL, NS, ag.grid_values, ag.grid_len, ag.grid_div, sh.cur_states, q);   // the generic rule
        } else {
            for (int i = 0; i < NS; i++) s[i] = ev.states[(size_t)e * NS + i];
            for (int i = 0; i < NANT; i++) sh.q_ant[i] = ev.q_ant[(size_t)e * NANT + i];
            env_do_action(ag.env_kind, sh.q_ant[NS], s, sh.cur_states);                                   // :97
            env_get_reward(ag.env_kind, sh.cur_states, sh.reward, sh.success);                            // :106
            env_quantize(ag.env_kind, NS, ag.grid_values, ag.grid_len, ag.grid_div, sh.cur_states, q);   // :112
        }
        for (int i = 0; i < NS; i++) sh.cur_q_ant[i] = q[i];
    }
    if ((int)threadIdx.x < ag.A) gs.ave[threadIdx.x] = ag.action_ve[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < NANT) sh.ve1[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, sh.q_ant[threadIdx.x]);
    if (threadIdx.x < NS) sh.ve2[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, sh.cur_q_ant[threadIdx.x]);
    __syncthreads();
    double q[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) q[k] = sh.ve2[k];
    double *base = rb + (size_t)e * (NANT + 1) * maxR;
    const double *qcol = base + (size_t)NANT * maxR;
    uint16_t *uidx_e = uidx ? uidx + (size_t)e * NANT * maxR : nullptr;
    const auto cols = ColsSel<IDX>::make(base, uidx_e, tab_s, maxR, U);
    double q1[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) q1[k] = sh.ve1[k];
    const auto pw = PowSel<PN, NANT>::make(ag.p > 0 ? ag.p : NANT);
    QResult rn;
    // one pass over the slab: greedy action for s' (:148) AND Q(s,a) of the pending update (frirl_update_sarsa.c:357)
    int ap;
    if constexpr (AMAX == 24) ap = sweep_gba_many<NANT, AMAX, BLOCK, true>(cols, qcol, nrules[e], q, q1, pw, ag.A, gs, red, &rn);
    else if constexpr (AMAX > 8) ap = sweep_gba_wide<NANT, 8, AMAX, BLOCK, true, TRACK>(cols, qcol, nrules[e], q, q1, pw, ag.A, gs, red, &rn, hp.weight_significant, cand_s);
    else {
        // the agent has not left its quantisation cell (workgroup-uniform): Q(s, a) of the pending update is the greedy sweep's conclusion
        // for action a at the new observation (sweeps.h: SAMES)
        bool same_cell = NS > 0 && FRIRL_STEP_SAME_CELL != 0;
#pragma unroll
        for (int k = 0; k < NS; k++) same_cell = same_cell && (q[k] == q1[k]);
        int apend = -1;
        for (int a = ag.A - 1; a >= 0; a--) if (gs.ave[a] == q1[NS]) apend = a;
        if (same_cell && apend >= 0) ap = sweep_gba_q<NANT, AMAX, BLOCK, TRACK, true>(cols, qcol, nrules[e], q, q1, pw, ag.A, gs, red, rn, hp.weight_significant, cand_s, apend);
        else ap = sweep_gba_q<NANT, AMAX, BLOCK, TRACK, false>(cols, qcol, nrules[e], q, q1, pw, ag.A, gs, red, rn, hp.weight_significant, cand_s);
    }
#ifdef FRIRL_STEP_TIMING
    const long long tm1 = wall_clock64();
#endif
    if (threadIdx.x == 0) {
        int chosen;
        if constexpr (EXT) chosen = e_greedy(ag, hp.epsilon, ap, (uint32_t)e, ev.episode ? (uint32_t)ev.episode[e] : 0u, (uint32_t)ev.ep_steps[e] + 1u);
        else chosen = e_greedy(ag, ap, (uint32_t)e, ev.episode ? (uint32_t)ev.episode[e] : 0u, (uint32_t)ev.ep_steps[e] + 1u);
        if constexpr (EXT) chosen = taught_action(io, e, ag.A, chosen);                               // :127-151: Q(s', a_teacher) below
        gs.best = chosen;
        // EXT under FRIRL_HIP_TARGET_Q (frirl_hip_target_rows): the update goes towards Q(s', g) of the greedy action `ap` the pick started
        // from, whatever the pick or the teacher chose; the episode goes on from (s', chosen) all the same
        if constexpr (EXT) { if ((io.tq.target ? (int)io.tq.target[e] : io.tq.target_all) == FRIRL_HIP_TARGET_Q) gs.best = ap; }
        // EXT under a set flag of frirl_hip_expect_rows: the update goes towards the expectation of the A conclusions under the pick at this
        // row's rate (frirl_hip.h), formed here from gs.actconc[] in action order; the target byte is then not consulted
        if constexpr (EXT) {
            double v = gs.actconc[gs.best];
            if (io.xp.expected ? (int)io.xp.expected[e] : io.xp.expected_all) {
                const double eps = ag.no_random == 1 ? 0.0 : hp.epsilon;
                v = gs.actconc[ap];
                if (eps != 0.0) {
                    double S = gs.actconc[0];
                    for (int a = 1; a < ag.A; a++) S = S + gs.actconc[a];
                    const double M = (S - 0.5 * gs.actconc[0]) + 0.5 * gs.actconc[ag.A - 1];
                    v = (1.0 - eps) * v + (eps / (double)ag.A) * M;
                }
            }
            qp_s = v;
        }
        sh.cur_q_ant[NS] = ag.grid_values[(size_t)NS * FRIRL_HIP_MAX_GRID + chosen];                  // :151
        sh.ve2[NS] = gs.ave[chosen];
        if constexpr (EXT) {
            io.action_out[e] = sh.cur_q_ant[NS];
            if (io.action_idx) io.action_idx[e] = chosen;
        }
    }
    __syncthreads();
    double qp;                                 // Q(s',a') of the chosen action == FIVE_vag_concl(cur_q_ant), frirl_update_sarsa.c:356 (EXT, target Q: Q(s', g))
    if constexpr (EXT) qp = qp_s; else qp = gs.actconc[gs.best];
    double *rant_e = ev.rant ? ev.rant + (size_t)e * NANT * maxR : nullptr;
    int st = FRIRL_HIP_UPD_INACTIVE;
    if (!ag.evaluate)                                                                                 // :155 (reduction_state == 0)
        st = update_sarsa_block_hp<NANT, BLOCK, TRACK>(cols, u, ve, U, base, maxR, nrules + e, ag, hp, sh, sh.reward, true, qp, ev.fus + e, rant_e, red, &rn, uidx_e, pw, cand_s,
                                                       ev.spread_ant ? ev.spread_ant + (size_t)e * NANT : nullptr, ev.spread_R ? ev.spread_R + e : nullptr);  // :159
    if (threadIdx.x < NS) ev.states[(size_t)e * NS + threadIdx.x] = sh.cur_states[threadIdx.x];      // :163-165
    if (threadIdx.x < NANT) ev.q_ant[(size_t)e * NANT + threadIdx.x] = sh.cur_q_ant[threadIdx.x];    // :166-168
    if (threadIdx.x == 0) {
        const int steps = ev.ep_steps[e] + 1;                                                         // :174
        ev.ep_steps[e] = steps;
        ev.ep_reward[e] = ev.ep_reward[e] + sh.reward;                                                // :107
        if (sh.success == 1 || steps >= ag.max_steps) ev.done[e] = 1;                                 // :183, :86
        if (ev.status) ev.status[e] = st;
#ifdef FRIRL_STEP_TIMING
        if (e < 65536) { g_step_timing[4 * e] = tm0; g_step_timing[4 * e + 1] = tm1; g_step_timing[4 * e + 2] = wall_clock64(); g_step_timing[4 * e + 3] = st; }
#endif
    }
}

template <int N, int AMAX, int BLOCK, bool BEGIN, bool EXT>
static void launch_episode_v(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                             hipStream_t s, const IoArg<EXT> &io)
{
    // compressed index mirror: large rule bases only (use_uidx); with one wave per environment only while the per-workgroup
    // LDS copy of the VE tables is small (<= 4 KiB: it does not limit the waves per CU)
    const bool idx = frirl::use_uidx(t, b) && (BLOCK >= 256 || sizeof(double) * t->nant * (size_t)t->U <= 4096);
    const size_t tab = idx ? sizeof(double) * t->nant * (size_t)t->U : 0;
    const bool pn = ag->p <= 0 || ag->p == N;                     // the Shepard power is the default nant: straight-line power (PowC<N>)
    // Spread candidates tracked in the fused sweep (sweeps.h: SpreadCand): where the second sweep would be a second pass over HBM
    // (large slabs) AND the sweep has registers to spare -- measured (tools/step_ab.py): acrobot 65 536 rules x 8 192 envs
    // 2.47 -> 2.26 ms per step; the 3-antecedent kernels (80-VGPR budget) and the 21-action kernel (already at 128) spill in the hot
    // loop with it (0.23 -> 0.57 ms, 3.0 -> 5.8 ms) and their second sweep is cheap beside A + 1 Shepard sums per rule, so they keep it.
    constexpr bool CAN_TRACK = (N >= 4 && AMAX <= 4);
    const int st_opt = frirl_host::opts().step_track;
    const bool track = CAN_TRACK && (st_opt == 1 || (st_opt < 0 && b->maxR > 16384 + 512));
#define EP_GO(KERNEL, DYN, ...)                                                                                                                  \
    hipLaunchKernelGGL((frirl::KERNEL<N, AMAX, BLOCK, __VA_ARGS__, EXT>), dim3(b->E), dim3(BLOCK), DYN, s, t->u, t->ve, t->U, b->rb, b->uidx, b->nrules, \
                       b->maxR, *ag, *ev, io)
    if constexpr (BEGIN) {
        if (idx) { if (pn) EP_GO(episode_begin_kernel, tab, true, true); else EP_GO(episode_begin_kernel, tab, true, false); }
        else { if (pn) EP_GO(episode_begin_kernel, 0, false, true); else EP_GO(episode_begin_kernel, 0, false, false); }
    } else {
        if constexpr (CAN_TRACK) {
            if (track) {
                if (idx) { if (pn) EP_GO(episode_step_kernel, tab, true, true, true); else EP_GO(episode_step_kernel, tab, true, false, true); }
                else { if (pn) EP_GO(episode_step_kernel, 0, false, true, true); else EP_GO(episode_step_kernel, 0, false, false, true); }
                return;
            }
        }
        if (idx) { if (pn) EP_GO(episode_step_kernel, tab, true, true, false); else EP_GO(episode_step_kernel, tab, true, false, false); }
        else { if (pn) EP_GO(episode_step_kernel, 0, false, true, false); else EP_GO(episode_step_kernel, 0, false, false, false); }
    }
#undef EP_GO
}

// Workgroup shape: 256 threads per environment for large rule bases (bandwidth); ONE wave per environment while
// the rule bases are small (<= 2048 rules: the demos' real learning regime, <= 367 rules) -- no cross-wave
// reductions or barriers on the critical path and 4x more environments resident per CU.  More than 8 actions
// always use 256 threads (the action-parallel sweep needs the waves).
template <int N, bool BEGIN, bool EXT = false>
static void launch_episode(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                           hipStream_t s, const IoArg<EXT> &io = IoArg<EXT>{})
{
    // one wave per environment: small rule bases, or mid-size ones when the environments alone fill the chip (>= 4 waves
    // per SIMD): measured at 8192 rules x 8192 envs 0.320 -> 0.295 ms per step; at 65 536 rules the 256-thread form wins
    bool small = b->maxR <= 2048 || (b->maxR <= 16384 && b->E >= 4096);
    // (1024 threads per environment -- fewer environments in flight, fewer concurrent DRAM streams -- measured slower at 65 536 rules:
    //  2.27 -> 2.79 ms per step, tools/step_ab.py)
    const int sw = frirl_host::opts().step_wave;
    if (sw >= 0) small = sw == 1;
    // (two waves per environment -- 16 384 half-size waves instead of 8192, a finer last round -- measured 0.225 vs 0.217 ms at 8192 x 8192)
    if (ag->A <= 4) { if (small) launch_episode_v<N, 4, 64, BEGIN, EXT>(t, b, ag, ev, s, io); else launch_episode_v<N, 4, 256, BEGIN, EXT>(t, b, ag, ev, s, io); }
    else if (ag->A <= 8) { if (small) launch_episode_v<N, 8, 64, BEGIN, EXT>(t, b, ag, ev, s, io); else launch_episode_v<N, 8, 256, BEGIN, EXT>(t, b, ag, ev, s, io); }
    else if (ag->A <= 24 && !frirl_host::opts().no_many) launch_episode_v<N, 24, 256, BEGIN, EXT>(t, b, ag, ev, s, io);   // 9..24 actions: all in registers (sweep_gba_many)
    else launch_episode_v<N, 32, 256, BEGIN, EXT>(t, b, ag, ev, s, io);            // more: action-parallel waves (sweep_gba_wide)
}

}  // namespace frirl
