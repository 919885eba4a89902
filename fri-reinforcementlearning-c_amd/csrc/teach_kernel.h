// teach_kernel.h -- one-launch replay of recorded demonstrations (frirl_hip_learn_demonstration, include/frirl_hip.h).
//
// One workgroup owns one agent and loops over the records of its log inside the kernel: per record the chain
// frirl_hip_agent_begin_taught / frirl_hip_agent_observe_taught would run (episode_kernel.h, EXT = true with every action forced),
// without a launch per record and without the A-way greedy sweep: the action at s' is the log's, so a record needs two
// conclusions, Q(s,a) of the pending update and Q(s',a'), and sweep_q_pair takes both from ONE read of each rule pair.
// Instantiated per antecedent count in teach_i<N>.hip.
#pragma once

#include "episode_kernel.h"

namespace frirl {

// sq_dist2's arithmetic (sweeps.h) on columns that are already loaded: dimension-ordered, first term a product, then one FMA each
template <int NDIM>
__device__ __forceinline__ void sq_dist2_loaded(const double2 (&v)[NDIM], const double (&q)[NDIM], double &a0, double &a1)
{
    double d0 = q[0] - v[0].x, d1 = q[0] - v[0].y;
    a0 = d0 * d0;
    a1 = d1 * d1;
#pragma unroll
    for (int k = 1; k < NDIM; k++) {
        d0 = q[k] - v[k].x;
        d1 = q[k] - v[k].y;
        a0 = __fma_rn(d0, d0, a0);
        a1 = __fma_rn(d1, d1, a1);
    }
}

// Two FIVE_vag_concl sweeps in one pass over the slab: `rn` for the point q1 = (s, a) (with the spread candidates under TRACK, as
// sweep_q<TRACK>) and `rp` for q2 = (s', a').  Each conclusion is sweep_q's: same lane mapping, same per-lane order, same block
// reduction, so either equals a separate sweep_q bit for bit.  SAME: the two points coincide (the agent stayed in its cell and
// repeated its action, workgroup-uniform) -- one conclusion serves both.
template <int NANT, int BLOCK, bool TRACK, bool SAME, class COLS, class POW>
__device__ void sweep_q_pair(const COLS &cols, const double *__restrict__ qcol, int R, const double (&q1)[NANT], const double (&q2)[NANT], POW p,
                             BlockRed<BLOCK> &red, QResult &rn, QResult &rp, double track_thr, SpreadCand *slot)
{
    unsigned best1 = FRIRL_HIP_NO_HIT, best2 = FRIRL_HIP_NO_HIT;
    double sv1 = 0.0, sw1 = 0.0, sv2 = 0.0, sw2 = 0.0;
    rn.tracked = TRACK;
    rp.tracked = false;
    if (TRACK) slot[threadIdx.x].clear();
    track_thr = wave_uniform(track_thr * SPREAD_PREFILTER_SLACK);
    double T = 0.0;
    const auto pk = pin_pow(p);
    const int r_lim = TRACK ? wave_uniform_limit(R) : R;      // tracked form: spread_track is a wave-level operation (sweep_q)
    for (int r = 2 * (int)threadIdx.x; r < r_lim; r += 2 * BLOCK) {
        double tw0 = 0.0, tw1 = 0.0;
        if (!TRACK || r < R) {
            double2 v[NANT];
#pragma unroll
            for (int k = 0; k < NANT; k++) v[k] = cols.pair(k, r);
            double2 c = load_col2(qcol + r);
            const bool second = (r + 1 < R);
            if (!second) c.y = 0.0;                             // the phantom rule of an odd tail: weight exactly 0 (sweep_q)
            double a0, a1;
            sq_dist2_loaded<NANT>(v, q1, a0, a1);
            if (!second) a1 = NO_RULE_STATE_PART;
            q_pair(a0, a1, c, (unsigned)r, pk, best1, sv1, sw1, tw0, tw1);
            if constexpr (!SAME) {
                double b0, b1, u0, u1;
                sq_dist2_loaded<NANT>(v, q2, b0, b1);
                if (!second) b1 = NO_RULE_STATE_PART;
                q_pair(b0, b1, c, (unsigned)r, pk, best2, sv2, sw2, u0, u1);
            }
        }
        if (TRACK) spread_track(slot, T, track_thr, tw0, tw1, (unsigned)r, sw1);
    }
    rn.hit = blk_min<BLOCK>(best1, red);
    rn.vagc = blk_sum<BLOCK>(sv1, red);
    rn.ws = blk_sum<BLOCK>(sw1, red);
    if constexpr (SAME) {
        rp.hit = rn.hit; rp.vagc = rn.vagc; rp.ws = rn.ws;
    } else {
        rp.hit = blk_min<BLOCK>(best2, red);
        rp.vagc = blk_sum<BLOCK>(sv2, red);
        rp.ws = blk_sum<BLOCK>(sw2, red);
    }
}

// what thread 0 decides about a record
enum : int { TEACH_STOP = 0, TEACH_START = 1, TEACH_SKIP = 2, TEACH_STEP = 3 };

struct TeachRow {       // the episode state of the agent while its log runs (frirl_hip_envs row e, written back once at the end)
    double ep_reward;
    int kind;
    int done, ep_steps, episode, status;
    int consumed, refused;
};

template <int NANT, int BLOCK, bool IDX, bool PN, bool TRACK>
__global__ __launch_bounds__(BLOCK) void teach_replay_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U, double *rb, uint16_t *uidx,
                                                             int32_t *nrules, int maxR, const frirl_hip_agent ag, const frirl_hip_envs ev,
                                                             const frirl_hip_demonstration dm, int passes, int32_t *replayed, uint8_t *refused)
{
    constexpr int NS = NANT - 1;
    const int e = blockIdx.x;
    extern __shared__ double tab_s[];
    __shared__ StepShared sh;
    __shared__ BlockRed<BLOCK> red;
    __shared__ SpreadCand cand_s[TRACK ? BLOCK : 1];
    __shared__ TeachRow row;
    if (IDX) for (int i = threadIdx.x; i < NANT * U; i += BLOCK) tab_s[i] = ve[i];
    int len = dm.T;
    if (dm.length) { len = dm.length[e]; len = len < 0 ? 0 : (len > dm.T ? dm.T : len); }
    const size_t off = (size_t)e * (size_t)dm.agent_stride;       // first record of this agent's log
    if (threadIdx.x == 0) {
        row.episode = ev.episode ? ev.episode[e] : 0;
        row.consumed = 0;
        row.refused = 0;
        row.kind = TEACH_STOP;
    }
    double *base = rb + (size_t)e * (NANT + 1) * maxR;
    double *qcol = base + (size_t)NANT * maxR;
    uint16_t *uidx_e = uidx ? uidx + (size_t)e * NANT * maxR : nullptr;
    double *rant_e = ev.rant ? ev.rant + (size_t)e * NANT * maxR : nullptr;
    const auto cols = ColsSel<IDX>::make(base, uidx_e, tab_s, maxR, U);
    const auto pw = PowSel<PN, NANT>::make(ag.p > 0 ? ag.p : NANT);
    bool stop = false;
    for (int pass = 0; pass < passes && !stop; pass++) {
        for (int r = 0; r < len; r++) {
            __syncthreads();      // the previous record is complete: its rule, consequents and row state are visible to every lane
            if (threadIdx.x == 0) {
                const size_t i = off + (size_t)r;
                const int a = dm.action[i];
                int kind;
                if (a < 0 || a >= ag.A) kind = TEACH_STOP;                               // the replay ends before this record
                else if (r == 0 || (dm.start && dm.start[i])) {
                    // frirl_hip_agent_begin_taught on this row: states = q_ant = obs, un-quantised (frirl_episode.c:46-48), the teacher's action (:58-79)
                    kind = TEACH_START;
                    for (int k = 0; k < NS; k++) { const double v = dm.obs[i * NS + k]; sh.cur_states[k] = v; sh.cur_q_ant[k] = v; }
                    sh.cur_q_ant[NS] = ag.grid_values[(size_t)NS * FRIRL_HIP_MAX_GRID + a];
                    row.episode = row.episode + 1;
                    row.done = 0;
                    row.ep_steps = 0;
                    row.ep_reward = 0.0;
                    row.status = FRIRL_HIP_UPD_INACTIVE;
                    row.consumed = row.consumed + 1;
                } else if (row.done) {
                    kind = TEACH_SKIP;                                                    // frirl_hip_agent_observe_taught skips a done row
                    row.status = FRIRL_HIP_UPD_INACTIVE;
                    row.consumed = row.consumed + 1;
                } else {
                    // frirl_hip_agent_observe_taught: the caller's do_action / get_reward / quantize_observations (:97-112) are the record
                    kind = TEACH_STEP;
                    double q[FRIRL_HIP_MAX_NANT];
                    for (int k = 0; k < NANT; k++) sh.q_ant[k] = sh.cur_q_ant[k];
                    for (int k = 0; k < NS; k++) sh.cur_states[k] = dm.obs[i * NS + k];
                    sh.reward = dm.reward[i];
                    sh.success = dm.success[i];
                    if (dm.q_obs) for (int k = 0; k < NS; k++) q[k] = dm.q_obs[i * NS + k];
                    else env_quantize(FRIRL_HIP_ENV_EXTERNAL, NS, ag.grid_values, ag.grid_len, ag.grid_div, sh.cur_states, q);
                    for (int k = 0; k < NS; k++) sh.cur_q_ant[k] = q[k];
                    sh.cur_q_ant[NS] = ag.grid_values[(size_t)NS * FRIRL_HIP_MAX_GRID + a];      // :151 with the teacher's action
                    sh.ve2[NS] = ag.action_ve[a];
                }
                row.kind = kind;
            }
            __syncthreads();
            const int kind = row.kind;
            if (kind == TEACH_STOP) { stop = true; break; }
            if (kind != TEACH_STEP) continue;
            if (threadIdx.x < NANT) sh.ve1[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, sh.q_ant[threadIdx.x]);
            if (threadIdx.x < NS) sh.ve2[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, sh.cur_q_ant[threadIdx.x]);
            __syncthreads();
            int st = FRIRL_HIP_UPD_INACTIVE;
            if (!ag.evaluate) {                                                           // :155 (reduction_state == 0)
                double q1[NANT], q2[NANT];
                bool same = true;
#pragma unroll
                for (int k = 0; k < NANT; k++) { q1[k] = sh.ve1[k]; q2[k] = sh.ve2[k]; same = same && (q1[k] == q2[k]); }
                const int R = nrules[e];
                QResult rn, rp;
                if (same) sweep_q_pair<NANT, BLOCK, TRACK, true>(cols, qcol, R, q1, q2, pw, red, rn, rp, ag.weight_significant, cand_s);
                else sweep_q_pair<NANT, BLOCK, TRACK, false>(cols, qcol, R, q1, q2, pw, red, rn, rp, ag.weight_significant, cand_s);
                const double qp = (rp.hit != FRIRL_HIP_NO_HIT) ? qcol[rp.hit] : rp.vagc / rp.ws;     // Q(s',a'), frirl_update_sarsa.c:356
                st = update_sarsa_block<NANT, BLOCK, TRACK>(cols, u, ve, U, base, maxR, nrules + e, ag, sh, sh.reward, true, qp, ev.fus + e, rant_e, red, &rn,
                                                            uidx_e, pw, cand_s, ev.spread_ant ? ev.spread_ant + (size_t)e * NANT : nullptr,
                                                            ev.spread_R ? ev.spread_R + e : nullptr);                      // :159
            }
            if (threadIdx.x == 0) {
                const int steps = row.ep_steps + 1;                                       // :174
                row.ep_steps = steps;
                row.ep_reward = row.ep_reward + sh.reward;                                // :107
                if (sh.success == 1 || steps >= ag.max_steps) row.done = 1;               // :183, :86
                row.status = st;
                if (st == FRIRL_HIP_UPD_FULL) row.refused = 1;
                row.consumed = row.consumed + 1;
            }
        }
    }
    __syncthreads();
    if (row.consumed > 0) {                  // record 0 was a start: every field below was set by the log
        if (threadIdx.x < NS) ev.states[(size_t)e * NS + threadIdx.x] = sh.cur_states[threadIdx.x];      // :163-165
        if (threadIdx.x < NANT) ev.q_ant[(size_t)e * NANT + threadIdx.x] = sh.cur_q_ant[threadIdx.x];    // :166-168
        if (threadIdx.x == 0) {
            if (ev.episode) ev.episode[e] = row.episode;
            ev.done[e] = row.done;
            ev.ep_steps[e] = row.ep_steps;
            ev.ep_reward[e] = row.ep_reward;
            if (ev.status) ev.status[e] = row.status;
        }
    }
    if (threadIdx.x == 0) {
        if (replayed) replayed[e] = row.consumed;
        if (refused) refused[e] = (uint8_t)row.refused;
    }
}

// Workgroup shape: one wave while maxR <= 2048, 256 threads beyond; the 16-bit index mirror with the LDS copy of the VE tables under
// launch_episode_v's rule (use_uidx needs maxR > 2048, so only the 256-thread form streams it); spread candidates tracked in the
// pair sweep where update_rules' second sweep would be a second pass over HBM (launch_episode_v: maxR > 16 896), at every
// antecedent count -- two conclusions per rule leave the registers for it.
template <int N>
static void launch_teach(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                         const frirl_hip_demonstration *dm, int passes, int32_t *replayed, uint8_t *refused, hipStream_t s)
{
    const bool pn = ag->p <= 0 || ag->p == N;
#define TEACH_GO(BLOCK, DYN, ...)                                                                                                                \
    hipLaunchKernelGGL((frirl::teach_replay_kernel<N, BLOCK, __VA_ARGS__>), dim3(b->E), dim3(BLOCK), DYN, s, t->u, t->ve, t->U, b->rb, b->uidx, b->nrules, \
                       b->maxR, *ag, *ev, *dm, passes, replayed, refused)
    if (b->maxR <= 2048) {
        if (pn) TEACH_GO(64, 0, false, true, false); else TEACH_GO(64, 0, false, false, false);
        return;
    }
    const bool idx = frirl::use_uidx(t, b);
    const size_t tab = idx ? sizeof(double) * t->nant * (size_t)t->U : 0;
    const int st_opt = frirl_host::opts().step_track;
    const bool track = st_opt == 1 || (st_opt < 0 && b->maxR > 16384 + 512);
    if (track) {
        if (idx) { if (pn) TEACH_GO(256, tab, true, true, true); else TEACH_GO(256, tab, true, false, true); }
        else { if (pn) TEACH_GO(256, 0, false, true, true); else TEACH_GO(256, 0, false, false, true); }
    } else {
        if (idx) { if (pn) TEACH_GO(256, tab, true, true, false); else TEACH_GO(256, tab, true, false, false); }
        else { if (pn) TEACH_GO(256, 0, false, true, false); else TEACH_GO(256, 0, false, false, false); }
    }
#undef TEACH_GO
}

}  // namespace frirl
