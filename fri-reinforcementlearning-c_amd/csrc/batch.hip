// batch.hip -- library-owned batch of E agents with host descriptors (frirl_hip_batch_*): what a plain-C host
// needs to run many agents on the GPU without touching the HIP runtime itself.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "batch_internal.h"
#include "device_common.h"

using namespace frirl_host;

struct frirl_hip_batch {
    int32_t nant, U, E, maxR;
    int device;                  // every entry point switches the calling thread to it (batches of several devices in one process)
    hipStream_t s;
    double *d_u, *d_ve, *d_rb, *d_rant, *d_grid, *d_ave, *d_states, *d_q_ant, *d_ep_reward, *d_start, *d_prev_reward, *d_prev_rconc, *d_tmp;
    uint16_t *d_uidx;            // 16-bit universe-index mirror of the antecedents (compressed scans, lane-group index store)
    double *d_weights;           // [E][maxR] FIVERB.weights of every agent (rule-base merge; allocated on first use)
    uint8_t *d_active;           // [E] receiver mask of a merge round
    int32_t *d_full;             // [E] append refused during a merge
    double *d_spread_ant;        // [E][nant] / [E]: what determines FIVERB.weights after learning (frirl_hip_envs.spread_*)
    int32_t *d_spread_R;
    void *d_lanes_ws;            // transposed rule bases of the lane-group kernel (allocated on first use)
    size_t lanes_ws_bytes;
    void *d_learn_ws;            // workspace of the persistent construct loop, frirl_hip_learn_train (allocated on first use)
    size_t learn_ws_bytes;
    int64_t *d_steps_total;      // [E] environment steps of the last frirl_hip_learn_train
    int32_t *d_nrules, *d_fus, *d_done, *d_ep_steps, *d_status, *d_episode, *d_prev_nrules, *d_prev_steps, *d_converged, *d_episodes, *d_epended;
    frirl_hip_tables t;
    frirl_hip_rulebases rb;
    frirl_hip_agent agent;
    frirl_hip_envs envs;
    frirl_hip_convergence conv;
    int64_t total_env_steps;
    double *d_hp;                // [5][E] per-agent hyper-parameter columns of frirl_hip_batch_set_hparams (allocated on first use) ...
    int32_t *d_hp_skip;          // [E]    ... and skip_rules
    frirl_hip_hparam_rows hp;    // the device columns that are set (all NULL: no rows)
    bool hp_set;
    double *d_ex_eps;            // [E] per-agent exploration columns of frirl_hip_batch_set_exploration (allocated on first use) ...
    int32_t *d_ex_h;             // [E] ... and horizons
    frirl_hip_explore_rows ex;   // the device columns that are set, and horizon_all
    bool ex_set;
    uint8_t *d_tq;               // [E] per-agent TD target of frirl_hip_batch_set_target (allocated on first use)
    frirl_hip_target_rows tq;    // the device column if one is set, and target_all
    bool tq_set;                 // a target other than SARSA for everybody is set
    uint8_t *d_xp;               // [E] per-agent expected-SARSA flags of frirl_hip_batch_set_expected (allocated on first use)
    frirl_hip_expect_rows xp;    // the device column if one is set, and expected_all
    bool xp_set;                 // flags other than 0 for everybody are set
    int32_t *d_evo;              // src, rank, status [E] each, then the read-back block of frirl_hip_batch_evolve_step (allocated on first use)
    uint32_t generation;         // successful evolve steps so far: keys the perturbation draws
    bool evo_scored;             // evo_successes / evo_reward hold the best agent's score of the last successful step
    int32_t evo_successes;
    double evo_reward;
    std::vector<int32_t> h_i;
    std::vector<double> h_d;
};

#define BCHK(call, what)                                                                                      \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e_)); return FRIRL_HIP_ELAUNCH; } \
    } while (0)

template <typename T>
static bool dalloc(T **p, size_t n)
{
    return hipMalloc((void **)p, n * sizeof(T)) == hipSuccess && hipMemset(*p, 0, n * sizeof(T)) == hipSuccess;
}

namespace frirl {
// done[e] |= converged[e]: converged agents sit later episodes out
__global__ void mask_converged_kernel(int32_t *__restrict__ done, const int32_t *__restrict__ converged, int E)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E && converged[e]) done[e] = 1;
}
// end of an exchange round: every agent but the master runs again in the next round whether or not its rule base was complete
// (frirl_sequential_run does not look at is_running on entry, frirl_agent.c:321-328), and `epended` starts every chunk at 0 (:37)
__global__ void next_round_kernel(int32_t *__restrict__ converged, int32_t *__restrict__ epended, int E, int first)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    epended[e] = 0;
    if (e >= first) converged[e] = 0;
}
// number of agents whose episode is still running -> *out
__global__ void count_running_kernel(const int32_t *__restrict__ done, int E, int32_t *__restrict__ out)
{
    int n = 0;
    for (int e = threadIdx.x; e < E; e += blockDim.x) n += done[e] ? 0 : 1;
    __shared__ int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    if (n) atomicAdd(&s, n);
    __syncthreads();
    if (threadIdx.x == 0) *out = s;
}
// frirl_hip_batch_teach: every student replays the whole log, everybody else nothing
__global__ void teach_lengths_kernel(const uint8_t *__restrict__ student, const int32_t *__restrict__ log_length, int E, int32_t *__restrict__ length)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) length[e] = student[e] ? log_length[0] : 0;
}
// after the replay: a student's convergence state is cleared as convergence_kernel's init clears it (frirl_init.c:149-150), but its
// episode counter stays; one workgroup per agent
__global__ __launch_bounds__(256) void teach_reset_kernel(const uint8_t *__restrict__ student, const double *__restrict__ rb,
                                                          const int32_t *__restrict__ nrules, int maxR, int nant, const frirl_hip_convergence c)
{
    const int e = blockIdx.x;
    if (!student[e]) return;
    const double *qcol = rb + ((size_t)e * (nant + 1) + nant) * maxR;
    double *prev = c.prev_rconc + (size_t)e * maxR;
    for (int r = threadIdx.x; r < maxR; r += blockDim.x) prev[r] = qcol[r];
    if (threadIdx.x == 0) {
        c.prev_nrules[e] = nrules[e];
        c.prev_steps[e] = -1;
        c.prev_reward[e] = -1.0;
        c.converged[e] = 0;
        if (c.epended) c.epended[e] = 0;
    }
}
}  // namespace frirl

extern "C" void frirl_hip_batch_destroy(frirl_hip_batch *b)
{
    if (!b) return;
    DeviceGuard keep_device_;
    (void)hipSetDevice(b->device);
    if (b->s) (void)hipStreamSynchronize(b->s);
    void *ptrs[] = {b->d_u, b->d_ve, b->d_rb, b->d_rant, b->d_grid, b->d_ave, b->d_states, b->d_q_ant, b->d_ep_reward, b->d_start, b->d_prev_reward,
                    b->d_prev_rconc, b->d_tmp, b->d_nrules, b->d_fus, b->d_done, b->d_ep_steps, b->d_status, b->d_episode, b->d_prev_nrules,
                    b->d_prev_steps, b->d_converged, b->d_episodes, b->d_epended, b->d_uidx, b->d_lanes_ws, b->d_learn_ws, b->d_steps_total, b->d_weights, b->d_active, b->d_full, b->d_spread_ant, b->d_spread_R, b->d_hp, b->d_hp_skip, b->d_ex_eps, b->d_ex_h, b->d_tq, b->d_xp, b->d_evo};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (b->s) (void)hipStreamDestroy(b->s);
    delete b;
}

extern "C" frirl_hip_batch *frirl_hip_batch_create(const frirl_hip_batch_desc *d)
{
    if (!d || !d->u || !d->ve || !d->agent.grid_values || !d->agent.action_ve || !d->rant0 || !d->rconc0) { set_error("frirl_hip_batch_create: NULL pointer"); return nullptr; }
    if (d->nant < 2 || d->nant > 9 || d->U < 2 || d->E < 1 || d->maxR < 2 || d->R0 < 1 || d->R0 > d->maxR || d->agent.A < 1 || d->agent.A > FRIRL_HIP_MAX_ACTIONS) { set_error("frirl_hip_batch_create: bad sizes"); return nullptr; }
    DeviceGuard keep_device_;
    if (d->device_select == 1 && hipSetDevice(d->device) != hipSuccess) { set_error("frirl_hip_batch_create: hipSetDevice(%d) failed", d->device); (void)hipGetLastError(); return nullptr; }
    if (check_device()) return nullptr;
    frirl_hip_batch *b = new frirl_hip_batch();
    if (hipGetDevice(&b->device) != hipSuccess) b->device = 0;
    b->nant = d->nant; b->U = d->U; b->E = d->E; b->maxR = d->maxR + (d->maxR & 1);
    const size_t E = (size_t)b->E, n = (size_t)b->nant, M = (size_t)b->maxR, ns = n - 1;
    bool ok = hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking) == hipSuccess;
    ok = ok && dalloc(&b->d_u, n * d->U) && dalloc(&b->d_ve, n * d->U) && dalloc(&b->d_rb, E * (n + 1) * M) && dalloc(&b->d_rant, E * n * M);
    ok = ok && dalloc(&b->d_grid, (size_t)FRIRL_HIP_MAX_NANT * FRIRL_HIP_MAX_GRID) && dalloc(&b->d_ave, (size_t)FRIRL_HIP_MAX_ACTIONS);
    ok = ok && dalloc(&b->d_states, E * ns) && dalloc(&b->d_q_ant, E * n) && dalloc(&b->d_ep_reward, E) && dalloc(&b->d_prev_reward, E);
    ok = ok && dalloc(&b->d_prev_rconc, E * M) && dalloc(&b->d_tmp, E * (n + 1)) && dalloc(&b->d_nrules, E) && dalloc(&b->d_fus, E) && dalloc(&b->d_done, E);
    ok = ok && dalloc(&b->d_ep_steps, E) && dalloc(&b->d_status, E) && dalloc(&b->d_episode, E) && dalloc(&b->d_prev_nrules, E) && dalloc(&b->d_prev_steps, E);
    ok = ok && dalloc(&b->d_converged, E) && dalloc(&b->d_episodes, E + 1) && dalloc(&b->d_epended, E) && dalloc(&b->d_spread_ant, E * n) && dalloc(&b->d_spread_R, E);
    if (ok && d->U <= 65536) ok = dalloc(&b->d_uidx, E * n * M);
    if (ok && d->start_states) ok = dalloc(&b->d_start, E * ns) && hipMemcpy(b->d_start, d->start_states, sizeof(double) * E * ns, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_u, d->u, sizeof(double) * n * d->U, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_ve, d->ve, sizeof(double) * n * d->U, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_grid, d->agent.grid_values, sizeof(double) * n * FRIRL_HIP_MAX_GRID, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_ave, d->agent.action_ve, sizeof(double) * d->agent.A, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { set_error("frirl_hip_batch_create: HIP allocation/copy failed: %s", hipGetErrorString(hipGetLastError())); frirl_hip_batch_destroy(b); return nullptr; }
    b->t.nant = b->nant; b->t.U = b->U; b->t.u = b->d_u; b->t.ve = b->d_ve;
    b->rb.E = b->E; b->rb.maxR = b->maxR; b->rb.rb = b->d_rb; b->rb.nrules = b->d_nrules; b->rb.uidx = b->d_uidx;
    b->agent = d->agent;
    b->agent.grid_values = b->d_grid;
    b->agent.action_ve = b->d_ave;
    memset(&b->envs, 0, sizeof b->envs);
    b->envs.states = b->d_states; b->envs.q_ant = b->d_q_ant; b->envs.fus = b->d_fus; b->envs.done = b->d_done; b->envs.ep_steps = b->d_ep_steps;
    b->envs.ep_reward = b->d_ep_reward; b->envs.rant = b->d_rant; b->envs.status = b->d_status; b->envs.start_states = b->d_start; b->envs.episode = b->d_episode;
    b->envs.spread_ant = b->d_spread_ant; b->envs.spread_R = b->d_spread_R;
    b->conv.prev_nrules = b->d_prev_nrules; b->conv.prev_steps = b->d_prev_steps; b->conv.prev_reward = b->d_prev_reward; b->conv.prev_rconc = b->d_prev_rconc;
    b->conv.converged = b->d_converged; b->conv.episodes = b->d_episodes; b->conv.epended = b->d_epended;
    b->total_env_steps = 0;
    // initial rules through FIVE_add_rule, as FIVEInit does (every agent gets the same R0 rules)
    std::vector<double> stage(E * (n + 1));
    for (int r = 0; r < d->R0; r++) {
        for (size_t e = 0; e < E; e++) {
            for (size_t k = 0; k < n; k++) stage[e * n + k] = d->rant0[(size_t)r * n + k];
            stage[E * n + e] = d->rconc0[r];
        }
        if (hipMemcpyAsync(b->d_tmp, stage.data(), sizeof(double) * E * (n + 1), hipMemcpyHostToDevice, b->s) != hipSuccess ||
            five_hip_add_rule(&b->t, &b->rb, b->d_tmp, b->d_tmp + E * n, nullptr, b->d_rant, nullptr, b->s) != 0 ||
            hipStreamSynchronize(b->s) != hipSuccess) {
            frirl_hip_batch_destroy(b);
            return nullptr;
        }
    }
    if (frirl_hip_convergence_init(&b->rb, b->nant, &b->conv, b->s) != 0 || hipStreamSynchronize(b->s) != hipSuccess) { frirl_hip_batch_destroy(b); return nullptr; }
    return b;
}

// the calls that learn without honouring per-agent hyper-parameters refuse while rows are set (frirl_hip_batch_set_hparams)
static int refuse_rows(const frirl_hip_batch *b, const char *who)
{
    if (b->ex_set && !b->hp_set) {
        set_error("%s: per-agent exploration is set (frirl_hip_batch_set_exploration) and this call does not honour it: use frirl_hip_batch_train, or clear it", who);
        return FRIRL_HIP_EINVAL;
    }
    if (b->hp_set) {
        set_error("%s: per-agent hyper-parameters are set (frirl_hip_batch_set_hparams) and this call does not honour them: use frirl_hip_batch_train, or clear them", who);
        return FRIRL_HIP_EINVAL;
    }
    if (b->tq_set) {
        set_error("%s: a per-agent TD target is set (frirl_hip_batch_set_target) and this call does not honour it: use frirl_hip_batch_train, or clear it", who);
        return FRIRL_HIP_EINVAL;
    }
    if (!b->xp_set) return FRIRL_HIP_OK;
    set_error("%s: per-agent expected SARSA is set (frirl_hip_batch_set_expected) and this call does not honour it: use frirl_hip_batch_train, or clear it", who);
    return FRIRL_HIP_EINVAL;
}

extern "C" int frirl_hip_batch_episode(frirl_hip_batch *b)
{
    if (!b) { set_error("frirl_hip_batch_episode: NULL batch"); return FRIRL_HIP_EINVAL; }
    if (refuse_rows(b, "frirl_hip_batch_episode")) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    int rc = frirl_hip_episode_begin(&b->t, &b->rb, &b->agent, &b->envs, b->s);
    if (rc) return rc;
    hipLaunchKernelGGL(frirl::mask_converged_kernel, dim3((b->E + 255) / 256), dim3(256), 0, b->s, b->d_done, b->d_converged, b->E);
    const int chunk = 64;
    int32_t running = 1;
    // many agents / small rule bases: lane-group kernel, the whole episode in one launch (frirl_hip_episode_run_lanes)
    if (frirl_hip_lanes_preferred(b->nant, b->E, b->agent.A)) {
        if (!b->d_lanes_ws) {
            b->lanes_ws_bytes = frirl_hip_lanes_workspace_bytes(b->nant, b->E, b->maxR, b->agent.A);
            BCHK(hipMalloc(&b->d_lanes_ws, b->lanes_ws_bytes), "lane-group workspace");
        }
        if ((rc = frirl_hip_episode_run_lanes(&b->t, &b->rb, &b->agent, &b->envs, b->agent.max_steps, b->d_lanes_ws, b->lanes_ws_bytes, b->s))) return rc;
        running = 0;
    } else
    // small rule bases: whole episode in one launch out of LDS (frirl_hip_episode_run); environments that outgrow the
    // LDS slab come back not-done and finish through the step kernel below
    if (b->agent.A <= 8 && 2 * sizeof(double) * b->nant * (size_t)b->U <= 16 * 1024) {
        b->h_i.resize(b->E);
        BCHK(hipMemcpyAsync(b->h_i.data(), b->d_nrules, sizeof(int32_t) * b->E, hipMemcpyDeviceToHost, b->s), "nrules download");
        BCHK(hipStreamSynchronize(b->s), "nrules sync");
        int need = 0;
        for (int e = 0; e < b->E; e++) if (b->h_i[e] > need) need = b->h_i[e];
        need += 128;
        if (need <= 256) {      // measured: the LDS-resident form pays only while the slab leaves >= ~12 waves per CU
            if ((rc = frirl_hip_episode_run(&b->t, &b->rb, &b->agent, &b->envs, b->agent.max_steps, need <= 256 ? 256 : (need <= 512 ? 512 : 1024), b->s))) return rc;
            hipLaunchKernelGGL(frirl::count_running_kernel, dim3(1), dim3(256), 0, b->s, b->d_done, b->E, b->d_episodes + b->E);
            BCHK(hipMemcpyAsync(&running, b->d_episodes + b->E, sizeof(int32_t), hipMemcpyDeviceToHost, b->s), "running download");
            BCHK(hipStreamSynchronize(b->s), "episode sync");
        }
    }
    for (int done_steps = 0; done_steps < b->agent.max_steps && running > 0; done_steps += chunk) {
        const int nst = (b->agent.max_steps - done_steps < chunk) ? b->agent.max_steps - done_steps : chunk;
        if ((rc = frirl_hip_episode_steps(&b->t, &b->rb, &b->agent, &b->envs, nst, b->s))) return rc;
        hipLaunchKernelGGL(frirl::count_running_kernel, dim3(1), dim3(256), 0, b->s, b->d_done, b->E, b->d_episodes + b->E);
        BCHK(hipMemcpyAsync(&running, b->d_episodes + b->E, sizeof(int32_t), hipMemcpyDeviceToHost, b->s), "running download");
        BCHK(hipStreamSynchronize(b->s), "episode sync");
    }
    // account the steps of the agents that took part in this episode (converged ones keep ep_steps = 0)
    b->h_i.resize(b->E);
    BCHK(hipMemcpyAsync(b->h_i.data(), b->d_ep_steps, sizeof(int32_t) * b->E, hipMemcpyDeviceToHost, b->s), "steps download");
    BCHK(hipStreamSynchronize(b->s), "steps sync");
    for (int e = 0; e < b->E; e++) b->total_env_steps += b->h_i[e];
    if ((rc = frirl_hip_convergence_update(&b->rb, b->nant, &b->agent, &b->envs, &b->conv, b->s))) return rc;
    BCHK(hipStreamSynchronize(b->s), "convergence sync");
    return check_launch("frirl_hip_batch_episode");
}

// The whole construct loop on the device (frirl_hip_learn_train) where the persistent learner covers the shape: every agent runs its
// episodes at its own pace instead of the batch waiting for its longest episode, launch after launch.  Same agents, same results
// (both forms follow the reference's loop per agent); *episodes_run = the largest number of episodes an agent ran in this call.
static int batch_train_persistent(frirl_hip_batch *b, int32_t max_episodes, int32_t *episodes_run)
{
    const size_t E = (size_t)b->E;
    b->h_i.resize(2 * E);
    BCHK(hipMemcpy(b->h_i.data(), b->d_episodes, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "episodes download");
    BCHK(hipMemcpy(b->h_i.data() + E, b->d_converged, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "converged download");
    int before = 0;
    bool all = true;
    for (size_t e = 0; e < E; e++) if (!b->h_i[E + e]) { all = false; before = std::max(before, b->h_i[e]); }
    if (episodes_run) *episodes_run = 0;
    if (all || max_episodes < 2) return FRIRL_HIP_OK;
    if (!b->d_learn_ws) {
        b->learn_ws_bytes = frirl_hip_learn_train_workspace_bytes(b->nant, b->E, b->maxR, b->agent.A);
        BCHK(hipMalloc(&b->d_learn_ws, b->learn_ws_bytes), "learner workspace");
        BCHK(hipMalloc((void **)&b->d_steps_total, sizeof(int64_t) * E), "learner step counters");
    }
    BCHK(hipMemsetAsync(b->d_steps_total, 0, sizeof(int64_t) * E, b->s), "step counters");
    BCHK(hipMemsetD32Async((hipDeviceptr_t)b->d_done, 1, E, b->s), "episode flags");       // every agent is between two episodes here
    // agents that are still learning have all run `before` episodes (the per-episode form keeps them in step): up to max_episodes - 1 more
    int32_t launches = 0;
    frirl_hip_agent exploring = b->agent;
    exploring.no_random = 0;                // exploration rows ask for exploration, whatever the batch's own flag (which every other call keeps reading)
    int rc = learn_train_structs(&b->t, &b->rb, b->ex_set ? &exploring : &b->agent, b->hp_set ? &b->hp : nullptr, b->ex_set ? &b->ex : nullptr,
                                 b->tq_set ? &b->tq : nullptr, b->xp_set ? &b->xp : nullptr, &b->envs, &b->conv, 512, max_episodes + before, b->d_steps_total, b->d_learn_ws, b->learn_ws_bytes,
                                 &launches, b->s);
    if (rc) return rc;
    std::vector<int64_t> st(E);
    BCHK(hipMemcpy(st.data(), b->d_steps_total, sizeof(int64_t) * E, hipMemcpyDeviceToHost), "steps download");
    BCHK(hipMemcpy(b->h_i.data(), b->d_episodes, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "episodes download");
    int after = before;
    for (size_t e = 0; e < E; e++) { b->total_env_steps += st[e]; after = std::max(after, b->h_i[e]); }
    if (episodes_run) *episodes_run = after - before;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_train(frirl_hip_batch *b, int32_t max_episodes, int32_t *episodes_run)
{
    if (!b) { set_error("frirl_hip_batch_train: NULL batch"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    if (!b->agent.evaluate && b->d_uidx && frirl_hip_learn_supported(b->nant, b->U, b->agent.A, b->agent.p, b->agent.env_kind))
        return batch_train_persistent(b, max_episodes, episodes_run);
    int ep = 0;
    for (ep = 1; ep < max_episodes; ep++) {             // at most max_episodes-1 episodes (frirl_sequential_run.c:51,59)
        int rc = frirl_hip_batch_episode(b);
        if (rc) return rc;
        b->h_i.resize(b->E);
        BCHK(hipMemcpy(b->h_i.data(), b->d_converged, sizeof(int32_t) * b->E, hipMemcpyDeviceToHost), "converged download");
        bool all = true;
        for (int e = 0; e < b->E && all; e++) all = b->h_i[e] != 0;
        if (all) { ep++; break; }
    }
    if (episodes_run) *episodes_run = ep - 1;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_stats(frirl_hip_batch *b, frirl_hip_batch_stats_t *out) { return frirl_host::batch_stats_first(b, out, nullptr); }

// the same + "agent 0's rule base is complete" from the same download (the multi-device report's master flag)
int frirl_host::batch_stats_first(frirl_hip_batch *b, frirl_hip_batch_stats_t *out, int32_t *first_converged)
{
    if (!b || !out) { set_error("frirl_hip_batch_stats: NULL"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const int E = b->E;
    std::vector<double> rew(E);
    std::vector<int32_t> steps(E), nr(E), cv(E), eps(E);
    BCHK(hipMemcpy(rew.data(), b->d_prev_reward, sizeof(double) * E, hipMemcpyDeviceToHost), "stats download");   // last finished episode
    BCHK(hipMemcpy(steps.data(), b->d_prev_steps, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "stats download");
    BCHK(hipMemcpy(nr.data(), b->d_nrules, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "stats download");
    BCHK(hipMemcpy(cv.data(), b->d_converged, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "stats download");
    BCHK(hipMemcpy(eps.data(), b->d_episodes, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "stats download");
    memset(out, 0, sizeof *out);
    out->agents = E;
    out->reward_min = rew[0]; out->reward_max = rew[0];
    for (int e = 0; e < E; e++) {
        out->reward_sum += rew[e]; out->steps_sum += steps[e]; out->rules_sum += nr[e];
        if (rew[e] < out->reward_min) out->reward_min = rew[e];
        if (rew[e] > out->reward_max) out->reward_max = rew[e];
        out->converged += cv[e] != 0;
        out->full_agents += nr[e] >= b->maxR;
        if (eps[e] > out->episodes_max) out->episodes_max = eps[e];
    }
    out->total_env_steps = b->total_env_steps;
    if (first_converged) *first_converged = cv[0];
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_agent_report(frirl_hip_batch *b, int32_t *converged, int32_t *episodes, int32_t *rules, int32_t *ep_steps, double *ep_reward)
{
    if (!b) { set_error("frirl_hip_batch_agent_report: NULL batch"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t E = (size_t)b->E;
    BCHK(hipStreamSynchronize(b->s), "report sync");
    if (converged) BCHK(hipMemcpy(converged, b->d_converged, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "report download");
    if (episodes) BCHK(hipMemcpy(episodes, b->d_episodes, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "report download");
    if (rules) BCHK(hipMemcpy(rules, b->d_nrules, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "report download");
    if (ep_steps) BCHK(hipMemcpy(ep_steps, b->d_prev_steps, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "report download");      // last finished episode
    if (ep_reward) BCHK(hipMemcpy(ep_reward, b->d_prev_reward, sizeof(double) * E, hipMemcpyDeviceToHost), "report download");
    return FRIRL_HIP_OK;
}

// what a valid set of per-agent hyper-parameters is (include/frirl_hip.h): host columns [E], no device
static int rows_check(const char *who, const frirl_hip_hparam_rows &h, int E, const frirl_hip_agent &agent)
{
    const double *cols[5] = {h.alpha, h.gamma, h.qdiff_pos_boundary, h.qdiff_neg_boundary, h.weight_significant};
    static const char *names[5] = {"alpha", "gamma", "qdiff_pos_boundary", "qdiff_neg_boundary", "weight_significant"};
    for (int e = 0; e < E; e++) {
        for (int c = 0; c < 5; c++)
            if (cols[c] && !(cols[c][e] - cols[c][e] == 0.0)) { set_error("%s: agent %d: %s is not finite", who, e, names[c]); return FRIRL_HIP_EINVAL; }
        const double pos = h.qdiff_pos_boundary ? h.qdiff_pos_boundary[e] : agent.qdiff_pos_boundary;
        const double neg = h.qdiff_neg_boundary ? h.qdiff_neg_boundary[e] : agent.qdiff_neg_boundary;
        if ((h.qdiff_pos_boundary || h.qdiff_neg_boundary) && !(pos >= neg)) {
            set_error("%s: agent %d: qdiff_pos_boundary %g < qdiff_neg_boundary %g", who, e, pos, neg);
            return FRIRL_HIP_EINVAL;
        }
        if (h.weight_significant && !(h.weight_significant[e] >= 0.0)) { set_error("%s: agent %d: weight_significant %g is negative", who, e, h.weight_significant[e]); return FRIRL_HIP_EINVAL; }
        if (h.skip_rules && h.skip_rules[e] != 0 && h.skip_rules[e] != 1) { set_error("%s: agent %d: skip_rules %d is neither 0 nor 1", who, e, h.skip_rules[e]); return FRIRL_HIP_EINVAL; }
    }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_hparam_rows_check(const frirl_hip_hparam_rows *host_rows, int32_t E, const frirl_hip_agent *agent)
{
    if (E < 1 || !agent) { set_error("frirl_hip_hparam_rows_check: E=%d / NULL agent", E); return FRIRL_HIP_EINVAL; }
    return host_rows ? rows_check("frirl_hip_hparam_rows_check", *host_rows, E, *agent) : FRIRL_HIP_OK;
}

// Per-agent hyper-parameter columns for frirl_hip_batch_train (include/frirl_hip.h): validated on the host, then copied.
extern "C" int frirl_hip_batch_set_hparams(frirl_hip_batch *b, const frirl_hip_hparam_rows *host_rows)
{
    static const char *who = "frirl_hip_batch_set_hparams";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    const frirl_hip_hparam_rows none = {};
    const frirl_hip_hparam_rows &h = host_rows ? *host_rows : none;
    const double *cols[5] = {h.alpha, h.gamma, h.qdiff_pos_boundary, h.qdiff_neg_boundary, h.weight_significant};
    if (!cols[0] && !cols[1] && !cols[2] && !cols[3] && !cols[4] && !h.skip_rules) {          // clear
        b->hp = none;
        b->hp_set = false;
        return FRIRL_HIP_OK;
    }
    if (!b->d_uidx || !frirl_hip_learn_supported(b->nant, b->U, b->agent.A, b->agent.p, b->agent.env_kind)) {
        set_error("%s: only the persistent learner takes per-agent hyper-parameters, and it does not cover this batch (frirl_hip_learn_supported: nant=%d U=%d A=%d p=%d; "
                  "index mirror: %s)", who, b->nant, b->U, b->agent.A, b->agent.p, b->d_uidx ? "yes" : "no");
        return FRIRL_HIP_EINVAL;
    }
    const int E = b->E;
    if (rows_check(who, h, E, b->agent)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    if (!b->d_hp) {
        if (!dalloc(&b->d_hp, (size_t)5 * E) || !dalloc(&b->d_hp_skip, (size_t)E)) { set_error("%s: HIP allocation failed: %s", who, hipGetErrorString(hipGetLastError())); return FRIRL_HIP_ELAUNCH; }
    }
    BCHK(hipStreamSynchronize(b->s), "hyper-parameter sync");           // nothing in flight reads the columns being replaced
    for (int c = 0; c < 5; c++)
        if (cols[c]) BCHK(hipMemcpy(b->d_hp + (size_t)c * E, cols[c], sizeof(double) * E, hipMemcpyHostToDevice), "hyper-parameter upload");
    if (h.skip_rules) BCHK(hipMemcpy(b->d_hp_skip, h.skip_rules, sizeof(int32_t) * E, hipMemcpyHostToDevice), "hyper-parameter upload");
    b->hp.alpha = cols[0] ? b->d_hp : nullptr;
    b->hp.gamma = cols[1] ? b->d_hp + (size_t)E : nullptr;
    b->hp.qdiff_pos_boundary = cols[2] ? b->d_hp + (size_t)2 * E : nullptr;
    b->hp.qdiff_neg_boundary = cols[3] ? b->d_hp + (size_t)3 * E : nullptr;
    b->hp.weight_significant = cols[4] ? b->d_hp + (size_t)4 * E : nullptr;
    b->hp.skip_rules = h.skip_rules ? b->d_hp_skip : nullptr;
    b->hp_set = true;
    return FRIRL_HIP_OK;
}

// what a valid set of per-agent exploration rows is (include/frirl_hip.h): host columns [E], no device
static int explore_check(const char *who, const frirl_hip_explore_rows &x, int E, const frirl_hip_agent &agent)
{
    const int32_t hmax = 1 << 30;
    if (x.reserved != 0) { set_error("%s: reserved is %d, not 0", who, x.reserved); return FRIRL_HIP_EINVAL; }
    if (x.horizon_all < 0 || x.horizon_all > hmax) { set_error("%s: horizon_all %d outside 0..2^30", who, x.horizon_all); return FRIRL_HIP_EINVAL; }
    if (!x.epsilon && !(agent.epsilon >= 0.0 && agent.epsilon <= 1.0)) { set_error("%s: the agent's epsilon %g (no epsilon column) is not in [0, 1]", who, agent.epsilon); return FRIRL_HIP_EINVAL; }
    for (int e = 0; e < E; e++) {
        if (x.epsilon && !(x.epsilon[e] >= 0.0 && x.epsilon[e] <= 1.0)) { set_error("%s: agent %d: epsilon %g is not in [0, 1]", who, e, x.epsilon[e]); return FRIRL_HIP_EINVAL; }
        if (x.horizon && (x.horizon[e] < 0 || x.horizon[e] > hmax)) { set_error("%s: agent %d: horizon %d outside 0..2^30", who, e, x.horizon[e]); return FRIRL_HIP_EINVAL; }
    }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_explore_rows_check(const frirl_hip_explore_rows *host_rows, int32_t E, const frirl_hip_agent *agent)
{
    if (E < 1 || !agent) { set_error("frirl_hip_explore_rows_check: E=%d / NULL agent", E); return FRIRL_HIP_EINVAL; }
    return host_rows ? explore_check("frirl_hip_explore_rows_check", *host_rows, E, *agent) : FRIRL_HIP_OK;
}

// Per-agent exploration for frirl_hip_batch_train (include/frirl_hip.h): validated on the host, then copied.
extern "C" int frirl_hip_batch_set_exploration(frirl_hip_batch *b, const frirl_hip_explore_rows *host_rows)
{
    static const char *who = "frirl_hip_batch_set_exploration";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (!host_rows) {                                                                          // clear
        b->ex = frirl_hip_explore_rows{};
        b->ex_set = false;
        return FRIRL_HIP_OK;
    }
    if (!b->d_uidx || !frirl_hip_learn_supported(b->nant, b->U, b->agent.A, b->agent.p, b->agent.env_kind)) {
        set_error("%s: only the persistent learner takes per-agent exploration, and it does not cover this batch (frirl_hip_learn_supported: nant=%d U=%d A=%d p=%d; "
                  "index mirror: %s)", who, b->nant, b->U, b->agent.A, b->agent.p, b->d_uidx ? "yes" : "no");
        return FRIRL_HIP_EINVAL;
    }
    const int E = b->E;
    if (explore_check(who, *host_rows, E, b->agent)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    if (!b->d_ex_eps) {
        if (!dalloc(&b->d_ex_eps, (size_t)E) || !dalloc(&b->d_ex_h, (size_t)E)) { set_error("%s: HIP allocation failed: %s", who, hipGetErrorString(hipGetLastError())); return FRIRL_HIP_ELAUNCH; }
    }
    BCHK(hipStreamSynchronize(b->s), "exploration sync");               // nothing in flight reads the columns being replaced
    if (host_rows->epsilon) BCHK(hipMemcpy(b->d_ex_eps, host_rows->epsilon, sizeof(double) * E, hipMemcpyHostToDevice), "exploration upload");
    if (host_rows->horizon) BCHK(hipMemcpy(b->d_ex_h, host_rows->horizon, sizeof(int32_t) * E, hipMemcpyHostToDevice), "exploration upload");
    b->ex = frirl_hip_explore_rows{};
    b->ex.epsilon = host_rows->epsilon ? b->d_ex_eps : nullptr;
    b->ex.horizon = host_rows->horizon ? b->d_ex_h : nullptr;
    b->ex.horizon_all = host_rows->horizon_all;
    b->ex_set = true;
    return FRIRL_HIP_OK;
}

// what a valid per-agent TD target is (include/frirl_hip.h): host column [E], no device
static int target_check(const char *who, const frirl_hip_target_rows &x, int E)
{
    if (x.reserved != 0) { set_error("%s: reserved is %d, not 0", who, x.reserved); return FRIRL_HIP_EINVAL; }
    if (x.target_all != FRIRL_HIP_TARGET_SARSA && x.target_all != FRIRL_HIP_TARGET_Q) { set_error("%s: target_all %d is neither 0 (SARSA) nor 1 (Q)", who, x.target_all); return FRIRL_HIP_EINVAL; }
    for (int e = 0; e < E; e++)
        if (x.target && x.target[e] > FRIRL_HIP_TARGET_Q) { set_error("%s: agent %d: target %d is neither 0 (SARSA) nor 1 (Q)", who, e, (int)x.target[e]); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_target_rows_check(const frirl_hip_target_rows *host_rows, int32_t E)
{
    if (E < 1) { set_error("frirl_hip_target_rows_check: E=%d", E); return FRIRL_HIP_EINVAL; }
    return host_rows ? target_check("frirl_hip_target_rows_check", *host_rows, E) : FRIRL_HIP_OK;
}

// Per-agent TD target for frirl_hip_batch_train (include/frirl_hip.h): validated on the host, then copied.
extern "C" int frirl_hip_batch_set_target(frirl_hip_batch *b, const uint8_t *host_target, int32_t target_all)
{
    static const char *who = "frirl_hip_batch_set_target";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (!host_target && target_all == FRIRL_HIP_TARGET_SARSA) {                                // clear
        b->tq = frirl_hip_target_rows{};
        b->tq_set = false;
        return FRIRL_HIP_OK;
    }
    if (!b->d_uidx || !frirl_hip_learn_supported(b->nant, b->U, b->agent.A, b->agent.p, b->agent.env_kind)) {
        set_error("%s: only the persistent learner takes a per-agent TD target, and it does not cover this batch (frirl_hip_learn_supported: nant=%d U=%d A=%d p=%d; "
                  "index mirror: %s)", who, b->nant, b->U, b->agent.A, b->agent.p, b->d_uidx ? "yes" : "no");
        return FRIRL_HIP_EINVAL;
    }
    const int E = b->E;
    frirl_hip_target_rows host = {};
    host.target = host_target; host.target_all = target_all;
    if (target_check(who, host, E)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    if (host_target && !b->d_tq && !dalloc(&b->d_tq, (size_t)E)) { set_error("%s: HIP allocation failed: %s", who, hipGetErrorString(hipGetLastError())); return FRIRL_HIP_ELAUNCH; }
    BCHK(hipStreamSynchronize(b->s), "target sync");                    // nothing in flight reads the column being replaced
    if (host_target) BCHK(hipMemcpy(b->d_tq, host_target, sizeof(uint8_t) * E, hipMemcpyHostToDevice), "target upload");
    b->tq = frirl_hip_target_rows{};
    b->tq.target = host_target ? b->d_tq : nullptr;
    b->tq.target_all = target_all;
    b->tq_set = true;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_get_target(frirl_hip_batch *b, uint8_t *host_target)
{
    static const char *who = "frirl_hip_batch_get_target";
    if (!b || !host_target) { set_error("%s: NULL batch or host_target", who); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    BCHK(hipStreamSynchronize(b->s), "target sync");
    if (b->tq.target) BCHK(hipMemcpy(host_target, b->tq.target, sizeof(uint8_t) * (size_t)b->E, hipMemcpyDeviceToHost), "target download");
    else std::fill_n(host_target, b->E, (uint8_t)b->tq.target_all);
    return FRIRL_HIP_OK;
}

// what valid per-agent expected-SARSA flags are (include/frirl_hip.h): host column [E], no device
static int expect_check(const char *who, const frirl_hip_expect_rows &x, int E)
{
    if (x.reserved != 0) { set_error("%s: reserved is %u, not 0", who, x.reserved); return FRIRL_HIP_EINVAL; }
    if (x.expected_all != 0 && x.expected_all != 1) { set_error("%s: expected_all %d is neither 0 nor 1", who, x.expected_all); return FRIRL_HIP_EINVAL; }
    for (int e = 0; e < E; e++)
        if (x.expected && x.expected[e] > 1) { set_error("%s: agent %d: expected %d is neither 0 nor 1", who, e, (int)x.expected[e]); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_expect_rows_check(const frirl_hip_expect_rows *host_rows, int32_t E)
{
    if (E < 1) { set_error("frirl_hip_expect_rows_check: E=%d", E); return FRIRL_HIP_EINVAL; }
    return host_rows ? expect_check("frirl_hip_expect_rows_check", *host_rows, E) : FRIRL_HIP_OK;
}

// Per-agent expected SARSA for frirl_hip_batch_train (include/frirl_hip.h): validated on the host, then copied.
extern "C" int frirl_hip_batch_set_expected(frirl_hip_batch *b, const uint8_t *host_expected, int32_t expected_all)
{
    static const char *who = "frirl_hip_batch_set_expected";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (!host_expected && expected_all == 0) {                                                 // clear
        b->xp = frirl_hip_expect_rows{};
        b->xp_set = false;
        return FRIRL_HIP_OK;
    }
    if (!b->d_uidx || !frirl_hip_learn_supported(b->nant, b->U, b->agent.A, b->agent.p, b->agent.env_kind)) {
        set_error("%s: only the persistent learner takes per-agent expected SARSA, and it does not cover this batch (frirl_hip_learn_supported: nant=%d U=%d A=%d p=%d; "
                  "index mirror: %s)", who, b->nant, b->U, b->agent.A, b->agent.p, b->d_uidx ? "yes" : "no");
        return FRIRL_HIP_EINVAL;
    }
    const int E = b->E;
    frirl_hip_expect_rows host = {};
    host.expected = host_expected; host.expected_all = expected_all;
    if (expect_check(who, host, E)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    if (host_expected && !b->d_xp && !dalloc(&b->d_xp, (size_t)E)) { set_error("%s: HIP allocation failed: %s", who, hipGetErrorString(hipGetLastError())); return FRIRL_HIP_ELAUNCH; }
    BCHK(hipStreamSynchronize(b->s), "expected sync");                  // nothing in flight reads the column being replaced
    if (host_expected) BCHK(hipMemcpy(b->d_xp, host_expected, sizeof(uint8_t) * E, hipMemcpyHostToDevice), "expected upload");
    b->xp = frirl_hip_expect_rows{};
    b->xp.expected = host_expected ? b->d_xp : nullptr;
    b->xp.expected_all = expected_all;
    b->xp_set = true;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_get_expected(frirl_hip_batch *b, uint8_t *host_expected)
{
    static const char *who = "frirl_hip_batch_get_expected";
    if (!b || !host_expected) { set_error("%s: NULL batch or host_expected", who); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    BCHK(hipStreamSynchronize(b->s), "expected sync");
    if (b->xp.expected) BCHK(hipMemcpy(host_expected, b->xp.expected, sizeof(uint8_t) * (size_t)b->E, hipMemcpyDeviceToHost), "expected download");
    else std::fill_n(host_expected, b->E, (uint8_t)b->xp.expected_all);
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_get_rulebase(frirl_hip_batch *b, int32_t e, int32_t *R, double *rant, double *rconc)
{
    if (!b || !R || e < 0 || e >= b->E) { set_error("frirl_hip_batch_get_rulebase: bad arguments"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    int32_t r = 0;
    BCHK(hipMemcpy(&r, b->d_nrules + e, sizeof(int32_t), hipMemcpyDeviceToHost), "nrules download");
    *R = r;
    if (!rant || !rconc || r == 0) return FRIRL_HIP_OK;
    const size_t n = b->nant, M = b->maxR;
    std::vector<double> col(r);
    for (size_t k = 0; k < n; k++) {
        BCHK(hipMemcpy(col.data(), b->d_rant + ((size_t)e * n + k) * M, sizeof(double) * r, hipMemcpyDeviceToHost), "rant download");
        for (int i = 0; i < r; i++) rant[(size_t)i * n + k] = col[i];
    }
    BCHK(hipMemcpy(rconc, b->d_rb + ((size_t)e * (n + 1) + n) * M, sizeof(double) * r, hipMemcpyDeviceToHost), "rconc download");
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reduce(frirl_hip_batch *b, int32_t e, int strategy, double reward_tolerance, int depth, frirl_hip_reduce_result *result)
{
    if (!b || !result || e < 0 || e >= b->E) { set_error("frirl_hip_batch_reduce: bad arguments"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t n = b->nant, M = b->maxR;
    frirl_hip_rulebases one = b->rb;                                 // agent e's slab as a rule-base batch of one
    one.E = 1;
    one.rb = b->d_rb + (size_t)e * (n + 1) * M;
    one.nrules = b->d_nrules + e;
    if (one.uidx) one.uidx = b->rb.uidx + (size_t)e * n * M;
    return frirl_hip_reduce_shared(&b->t, &one, &b->agent, b->d_rant + (size_t)e * n * M, strategy, reward_tolerance, depth, nullptr, result, b->s);
}

extern "C" int frirl_hip_batch_reduce_all(frirl_hip_batch *b, int strategy, double reward_tolerance, int depth, frirl_hip_reduce_result *results,
                                          int32_t *agents_reduced)
{
    if (!b) { set_error("frirl_hip_batch_reduce_all: NULL batch"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    std::vector<frirl_hip_reduce_result> res(b->E);
    const size_t bytes = frirl_hip_reduce_batch_workspace_bytes(b->nant, b->E, b->maxR, depth);
    void *ws = nullptr;
    if (bytes) BCHK(hipMalloc(&ws, bytes), "reduction workspace");      // bytes == 0: a bad depth, refused below
    const int rc = frirl_hip_reduce_batch(&b->t, &b->rb, &b->agent, b->d_rant, b->d_start, nullptr, strategy, reward_tolerance, depth, nullptr, res.data(),
                                          ws, bytes, b->s);
    if (ws) (void)hipFree(ws);
    if (rc) return rc;
    int32_t n = 0;
    for (int e = 0; e < b->E; e++) n += res[e].rules_after < res[e].rules_before;
    if (results) memcpy(results, res.data(), sizeof(frirl_hip_reduce_result) * b->E);
    if (agents_reduced) *agents_reduced = n;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reduce_all_starts(frirl_hip_batch *b, int strategy, double reward_tolerance, int depth, int32_t n, const double *start_states,
                                                 int drop_bad_starts, frirl_hip_reduce_result *results, frirl_hip_reduce_start_result *per_start,
                                                 int32_t *agents_reduced)
{
    static const char *who = "frirl_hip_batch_reduce_all_starts";
    if (!b || !start_states) { set_error("%s: NULL batch or start states", who); return FRIRL_HIP_EINVAL; }
    if (n < 1 || n > FRIRL_HIP_REDUCE_MAX_STARTS) { set_error("%s: n=%d start states outside 1..%d", who, n, FRIRL_HIP_REDUCE_MAX_STARTS); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    std::vector<frirl_hip_reduce_result> res(b->E);
    const size_t bytes = frirl_hip_reduce_batch_starts_workspace_bytes(b->nant, b->E, b->maxR, depth, n);      // 0: a bad depth, refused below
    const size_t sbytes = (sizeof(double) * (size_t)b->E * n * (b->nant - 1) + 15) / 16 * 16;
    char *mem = nullptr;
    BCHK(hipMalloc(reinterpret_cast<void **>(&mem), sbytes + bytes), "reduction workspace");
    hipError_t up = hipMemcpyAsync(mem, start_states, sizeof(double) * (size_t)b->E * n * (b->nant - 1), hipMemcpyHostToDevice, b->s);
    if (up == hipSuccess) up = hipStreamSynchronize(b->s);             // start_states is the caller's pageable memory
    if (up != hipSuccess) { (void)hipFree(mem); set_error("%s: start states upload: %s", who, hipGetErrorString(up)); return FRIRL_HIP_ELAUNCH; }
    frirl_hip_reduce_starts st = {};
    st.n = n;
    st.drop_bad_starts = drop_bad_starts;
    st.start_states = reinterpret_cast<const double *>(mem);
    const int rc = frirl_hip_reduce_batch_starts(&b->t, &b->rb, &b->agent, b->d_rant, &st, nullptr, strategy, reward_tolerance, depth, nullptr, res.data(),
                                                 per_start, bytes ? mem + sbytes : nullptr, bytes, b->s);
    (void)hipFree(mem);
    if (rc) return rc;
    int32_t reduced = 0;
    for (int e = 0; e < b->E; e++) reduced += res[e].rules_after < res[e].rules_before;
    if (results) memcpy(results, res.data(), sizeof(frirl_hip_reduce_result) * b->E);
    if (agents_reduced) *agents_reduced = reduced;
    return FRIRL_HIP_OK;
}

// frirl_hip_batch_reduce_all_map (order_set == 0: `strategy`, results in `results`) and frirl_hip_batch_reduce_all_map_orders (order_set
// != 0: results in `ores` / `after_per_order`): the roll-out of the points, the bookkeeping and the totals are one piece of code
static int batch_reduce_all_map_run(const char *who, frirl_hip_batch *b, int strategy, int order_set, int32_t n, const double *start_states, int only_successful,
                                    int32_t cap, frirl_hip_reduce_map_result *results, frirl_hip_reduce_orders_result *ores, int32_t *after_per_order,
                                    frirl_hip_reduce_map_totals *totals)
{
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (n < 1 || n > FRIRL_HIP_REDUCE_MAX_STARTS) { set_error("%s: n=%d start states outside 1..%d", who, n, FRIRL_HIP_REDUCE_MAX_STARTS); return FRIRL_HIP_EINVAL; }
    if (!start_states && n != 1) { set_error("%s: NULL start states with n=%d (every agent's own start: n = 1)", who, n); return FRIRL_HIP_EINVAL; }
    if (!order_set && strategy != 1 && strategy != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy); return FRIRL_HIP_EINVAL; }
    if (cap < 0 || cap > FRIRL_HIP_POINTS_MAX_CAP) { set_error("%s: cap=%d outside 0..%d", who, cap, FRIRL_HIP_POINTS_MAX_CAP); return FRIRL_HIP_EINVAL; }
    if (cap == 0) cap = FRIRL_HIP_POINTS_MAX_CAP;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t E = (size_t)b->E, ns = (size_t)b->nant - 1, Q = E * (size_t)n, M = (size_t)b->maxR;
    const int K = __builtin_popcount((unsigned)order_set);
    const bool usage = (order_set & 12) != 0;
    const size_t ws_points = frirl_hip_rollout_points_workspace_bytes(b->nant, b->E, b->maxR, n, cap, b->agent.A);
    const size_t ws_map = order_set ? frirl_hip_reduce_batch_map_orders_workspace_bytes(b->nant, b->E, b->maxR, cap, K)
                                    : frirl_hip_reduce_batch_map_workspace_bytes(b->nant, b->E, b->maxR, cap);
    const size_t ws_usage = usage ? frirl_hip_rule_usage_workspace_bytes(b->nant, b->E, cap) : 0;
    const size_t ws_bytes = std::max(ws_points, std::max(ws_map, ws_usage));   // the calls follow each other on one stream
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
    const size_t o_ws = take(ws_bytes), o_points = take(sizeof(double) * E * (size_t)cap * ns), o_start = take(start_states ? sizeof(double) * Q * ns : 0);
    const size_t o_count = take(sizeof(int32_t) * E), o_over = take(sizeof(int32_t) * E), o_active = take(E);
    const size_t o_sum = take(usage ? sizeof(double) * E * M : 0), o_one = take(order_set ? sizeof(int32_t) * E * M : 0);
    const size_t o_orders = take(sizeof(int32_t) * E * M * (size_t)K);
    char *mem = nullptr;
    BCHK(hipMalloc(reinterpret_cast<void **>(&mem), off), "map reduction buffers");
    frirl_hip_rollout_points_desc rp = {};
    rp.n = n; rp.cap = cap; rp.only_successful = only_successful ? 1 : 0;
    rp.start_states = start_states ? reinterpret_cast<const double *>(mem + o_start) : b->d_start;   // n == 1: the batch's own [E][nant-1], or values_def
    rp.points = reinterpret_cast<double *>(mem + o_points);
    rp.point_count = reinterpret_cast<int32_t *>(mem + o_count);
    rp.overflow = reinterpret_cast<int32_t *>(mem + o_over);
    frirl_hip_agent greedy = b->agent;
    greedy.no_random = 1;                                             // the points of the GREEDY policy (frirl_test_run: reduction_state == 1)
    std::vector<int32_t> count(E), over(E);
    std::vector<uint8_t> active(E);
    std::vector<frirl_hip_reduce_map_result> res(E);
    std::vector<frirl_hip_reduce_orders_result> resk(order_set ? E : 0);
    int rc = FRIRL_HIP_OK;
    hipError_t he = hipSuccess;
    if (start_states) he = hipMemcpyAsync(mem + o_start, start_states, sizeof(double) * Q * ns, hipMemcpyHostToDevice, b->s);
    if (he == hipSuccess) rc = frirl_hip_rollout_points(&b->t, &b->rb, &greedy, &rp, mem + o_ws, ws_bytes, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemcpyAsync(count.data(), rp.point_count, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemcpyAsync(over.data(), rp.overflow, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s);
    if (he == hipSuccess) he = hipStreamSynchronize(b->s);            // also on failure of the call: `start_states` may be in use by the upload
    else (void)hipStreamSynchronize(b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) {
        for (size_t e = 0; e < E; e++) active[e] = over[e] ? 0 : 1;
        he = hipMemcpy(mem + o_active, active.data(), E, hipMemcpyHostToDevice);
    }
    if (he == hipSuccess && rc == FRIRL_HIP_OK) {
        frirl_hip_map_points mp = {};
        mp.n = cap;
        mp.points = rp.points;
        mp.point_count = rp.point_count;
        mp.active = reinterpret_cast<const uint8_t *>(mem + o_active);
        if (!order_set) rc = frirl_hip_reduce_batch_map(&b->t, &b->rb, &greedy, b->d_rant, &mp, strategy, nullptr, res.data(), mem + o_ws, ws_bytes, b->s);
        double *sum = reinterpret_cast<double *>(mem + o_sum);
        int32_t *one = reinterpret_cast<int32_t *>(mem + o_one), *orders = reinterpret_cast<int32_t *>(mem + o_orders);
        if (usage) {
            const frirl_hip_rule_usage_out uo = {sum, nullptr, nullptr};
            rc = frirl_hip_rule_usage(&b->t, &b->rb, &greedy, &mp, &uo, mem + o_ws, ws_bytes, b->s);
        }
        // order k = the k-th set bit from the lowest: ranked into one [E][maxR] array, then interleaved into [E][K][maxR]
        for (int bit = 0, k = 0; bit < 4 && rc == FRIRL_HIP_OK && he == hipSuccess; bit++) {
            if (!(order_set >> bit & 1)) continue;
            rc = frirl_hip_rule_order(&b->rb, b->nant, bit < 2 ? nullptr : sum, bit & 1, mp.active, one, b->s);
            if (rc == FRIRL_HIP_OK)
                he = hipMemcpy2DAsync(orders + (size_t)k * M, sizeof(int32_t) * M * K, one, sizeof(int32_t) * M, sizeof(int32_t) * M, E, hipMemcpyDeviceToDevice, b->s);
            k += 1;
        }
        if (order_set && rc == FRIRL_HIP_OK && he == hipSuccess)
            rc = frirl_hip_reduce_batch_map_orders(&b->t, &b->rb, &greedy, b->d_rant, &mp, K, orders, nullptr, resk.data(), after_per_order, mem + o_ws, ws_bytes,
                                                   b->s);
        else if (order_set) (void)hipStreamSynchronize(b->s);
        for (size_t e = 0; order_set && e < E; e++) res[e] = {resk[e].rules_before, resk[e].rules_after, resk[e].points, resk[e].tries};
    }
    (void)hipFree(mem);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(he)); return FRIRL_HIP_ELAUNCH; }
    frirl_hip_reduce_map_totals tot = {};
    for (size_t e = 0; e < E; e++) {
        tot.agents_reduced += res[e].rules_after < res[e].rules_before;
        tot.agents_overflow += over[e] != 0;
        tot.agents_without_points += !over[e] && count[e] == 0;
        tot.rules_before += res[e].rules_before;
        tot.rules_after += res[e].rules_after;
        tot.points += over[e] ? 0 : count[e];
    }
    if (results) memcpy(results, res.data(), sizeof(frirl_hip_reduce_map_result) * E);
    if (ores) memcpy(ores, resk.data(), sizeof(frirl_hip_reduce_orders_result) * E);
    if (totals) *totals = tot;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reduce_all_map(frirl_hip_batch *b, int strategy, int32_t n, const double *start_states, int only_successful, int32_t cap,
                                              frirl_hip_reduce_map_result *results, frirl_hip_reduce_map_totals *totals)
{
    return batch_reduce_all_map_run("frirl_hip_batch_reduce_all_map", b, strategy, 0, n, start_states, only_successful, cap, results, nullptr, nullptr, totals);
}

extern "C" int frirl_hip_batch_reduce_all_map_orders(frirl_hip_batch *b, int order_set, int32_t n, const double *start_states, int only_successful, int32_t cap,
                                                     frirl_hip_reduce_orders_result *results, int32_t *after_per_order, frirl_hip_reduce_map_totals *totals)
{
    static const char *who = "frirl_hip_batch_reduce_all_map_orders";
    if (order_set < 1 || order_set > 15) {
        set_error("%s: order_set=%d outside 1..15 (1 = |Q| ascending, 2 = |Q| descending, 4 = usage ascending, 8 = usage descending)", who, order_set);
        return FRIRL_HIP_EINVAL;
    }
    return batch_reduce_all_map_run(who, b, 0, order_set, n, start_states, only_successful, cap, nullptr, results, after_per_order, totals);
}

// what frirl_hip_batch_evaluate refuses before it looks at the device
static int evaluate_args_check(const char *who, const frirl_hip_batch *b, int32_t n)
{
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (n < 1 || (int64_t)b->E * n > INT32_MAX) { set_error("%s: n=%d outside 1..INT32_MAX / E", who, n); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

// The device part of an evaluation: buffers allocated (q.mem, the caller frees it after synchronising), start states uploaded and the
// greedy roll-outs queued on b->s.  The scores stay on the device, [E] at the start of q.mem.  `he` takes a failed runtime call; the
// caller synchronises in every case, since `q.own` and `q.mem` may be in use by the upload.
struct EvalQueued {
    char *mem = nullptr;
    std::vector<double> own;
    frirl_hip_rollout_score *scores() const { return reinterpret_cast<frirl_hip_rollout_score *>(mem); }
};

static int batch_evaluate_queue(frirl_hip_batch *b, int32_t n, const double *start_states, EvalQueued &q, hipError_t &he)
{
    const size_t E = (size_t)b->E, ns = (size_t)b->nant - 1, Q = E * (size_t)n;
    // every row at the agent's own start: its desc.start_states row n times (agent.values_def where the batch has none: no array at all)
    if (!start_states && b->d_start) {
        std::vector<double> one(E * ns);
        BCHK(hipMemcpy(one.data(), b->d_start, sizeof(double) * E * ns, hipMemcpyDeviceToHost), "start states download");
        q.own.resize(Q * ns);
        for (size_t r = 0; r < Q; r++) memcpy(&q.own[r * ns], &one[(r / (size_t)n) * ns], sizeof(double) * ns);
        start_states = q.own.data();
    }
    const size_t ws_bytes = frirl_hip_rollout_batch_workspace_bytes(b->nant, b->E, b->maxR, n, b->agent.A);
    const size_t off_reward = (sizeof(frirl_hip_rollout_score) * E + 15) / 16 * 16, off_start = off_reward + sizeof(double) * Q;
    const size_t off_steps = off_start + (start_states ? sizeof(double) * Q * ns : 0), off_ws = (off_steps + sizeof(int32_t) * 2 * Q + 15) / 16 * 16;
    char *mem = nullptr;
    BCHK(hipMalloc(reinterpret_cast<void **>(&mem), off_ws + ws_bytes), "evaluation buffers");
    q.mem = mem;
    frirl_hip_rollout_batch_rows ro = {};
    ro.n = n;
    ro.reward = reinterpret_cast<double *>(mem + off_reward);
    ro.steps = reinterpret_cast<int32_t *>(mem + off_steps);
    ro.success = ro.steps + Q;
    frirl_hip_agent greedy = b->agent;
    greedy.no_random = 1;                                             // an evaluation is greedy (frirl_test_run: reduction_state == 1)
    int rc = FRIRL_HIP_OK;
    if (start_states) {
        ro.start_states = reinterpret_cast<double *>(mem + off_start);
        he = hipMemcpyAsync(mem + off_start, start_states, sizeof(double) * Q * ns, hipMemcpyHostToDevice, b->s);
    }
    if (he == hipSuccess) rc = frirl_hip_rollout_batch(&b->t, &b->rb, &greedy, &ro, q.scores(), mem + off_ws, ws_bytes, b->s);
    return rc;
}

extern "C" int frirl_hip_batch_evaluate(frirl_hip_batch *b, int32_t n, const double *start_states, frirl_hip_rollout_score *scores, int32_t *best)
{
    static const char *who = "frirl_hip_batch_evaluate";
    if (evaluate_args_check(who, b, n)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t E = (size_t)b->E;
    std::vector<frirl_hip_rollout_score> sc(E);
    EvalQueued q;
    hipError_t he = hipSuccess;
    const int rc = batch_evaluate_queue(b, n, start_states, q, he);
    if (!q.mem) return rc;                                            // nothing was queued
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemcpyAsync(sc.data(), q.mem, sizeof(frirl_hip_rollout_score) * E, hipMemcpyDeviceToHost, b->s);
    if (he == hipSuccess) he = hipStreamSynchronize(b->s);            // also on failure of the call: `q.own` and `q.mem` may be in use by the upload
    else (void)hipStreamSynchronize(b->s);
    (void)hipFree(q.mem);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(he)); return FRIRL_HIP_ELAUNCH; }
    int32_t win = 0;                                                  // most successes, then the largest reward_sum, then the lowest index
    for (int e = 1; e < b->E; e++)
        if (sc[e].successes > sc[win].successes || (sc[e].successes == sc[win].successes && sc[e].reward_sum > sc[win].reward_sum)) win = e;
    if (scores) memcpy(scores, sc.data(), sizeof(frirl_hip_rollout_score) * E);
    if (best) *best = win;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_teach(frirl_hip_batch *b, int32_t teacher, int32_t episodes, const double *start_states, int32_t passes,
                                     const uint8_t *students, frirl_hip_teach_result *result)
{
    static const char *who = "frirl_hip_batch_teach";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (refuse_rows(b, who)) return FRIRL_HIP_EINVAL;
    if (teacher < 0 || teacher >= b->E) { set_error("%s: teacher=%d outside 0..%d", who, teacher, b->E - 1); return FRIRL_HIP_EINVAL; }
    if (episodes < 1 || (int64_t)episodes * ((int64_t)b->agent.max_steps + 1) > INT32_MAX) { set_error("%s: episodes=%d outside 1..INT32_MAX / (max_steps + 1)", who, episodes); return FRIRL_HIP_EINVAL; }
    if (passes < 1 || passes > 1024) { set_error("%s: passes=%d outside 1..1024", who, passes); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    BCHK(hipStreamSynchronize(b->s), "teach sync");
    int32_t teacher_rules = 0;
    BCHK(hipMemcpy(&teacher_rules, b->d_nrules + teacher, sizeof teacher_rules, hipMemcpyDeviceToHost), "nrules download");
    if (teacher_rules < 1 || teacher_rules > b->maxR) { set_error("%s: teacher %d holds %d rules (capacity %d)", who, teacher, teacher_rules, b->maxR); return FRIRL_HIP_EINVAL; }
    const size_t E = (size_t)b->E, ns = (size_t)b->nant - 1, K = (size_t)episodes;
    const int64_t T64 = (int64_t)episodes * ((int64_t)b->agent.max_steps + 1);
    const size_t T = (size_t)(T64 < 2 ? 2 : T64);
    // episode k at the own start state of agent k % E (agent.values_def where the batch has none: no array at all)
    std::vector<double> own;
    if (!start_states && b->d_start) {
        std::vector<double> one(E * ns);
        BCHK(hipMemcpy(one.data(), b->d_start, sizeof(double) * E * ns, hipMemcpyDeviceToHost), "start states download");
        own.resize(K * ns);
        for (size_t k = 0; k < K; k++) memcpy(&own[k * ns], &one[(k % E) * ns], sizeof(double) * ns);
        start_states = own.data();
    }
    std::vector<uint8_t> mask(E);
    int32_t nstudents = 0;
    for (size_t e = 0; e < E; e++) {
        mask[e] = (e != (size_t)teacher && (!students || students[e])) ? 1 : 0;
        nstudents += mask[e];
    }
    // one allocation: doubles, then int32s, then bytes
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
    const size_t o_obs = take(sizeof(double) * T * ns), o_qobs = take(sizeof(double) * T * ns), o_reward = take(sizeof(double) * T);
    const size_t o_epr = take(sizeof(double) * K), o_st = take(sizeof(double) * K * ns);
    const size_t o_action = take(sizeof(int32_t) * T), o_success = take(sizeof(int32_t) * T), o_len = take(sizeof(int32_t));
    const size_t o_eps = take(sizeof(int32_t) * K), o_epok = take(sizeof(int32_t) * K), o_length = take(sizeof(int32_t) * E), o_replayed = take(sizeof(int32_t) * E);
    const size_t o_start = take(T), o_mask = take(E), o_refused = take(E);
    char *mem = nullptr;
    BCHK(hipMalloc(reinterpret_cast<void **>(&mem), off), "teaching buffers");
    frirl_hip_rollout_log lg = {};
    lg.n = 1; lg.episodes = episodes; lg.T = (int32_t)T;
    lg.obs = reinterpret_cast<double *>(mem + o_obs); lg.q_obs = reinterpret_cast<double *>(mem + o_qobs); lg.reward = reinterpret_cast<double *>(mem + o_reward);
    lg.action = reinterpret_cast<int32_t *>(mem + o_action); lg.success = reinterpret_cast<int32_t *>(mem + o_success);
    lg.start = reinterpret_cast<uint8_t *>(mem + o_start); lg.length = reinterpret_cast<int32_t *>(mem + o_len);
    lg.ep_steps = reinterpret_cast<int32_t *>(mem + o_eps); lg.ep_reward = reinterpret_cast<double *>(mem + o_epr); lg.ep_success = reinterpret_cast<int32_t *>(mem + o_epok);
    int32_t *d_length = reinterpret_cast<int32_t *>(mem + o_length), *d_replayed = reinterpret_cast<int32_t *>(mem + o_replayed);
    uint8_t *d_mask = reinterpret_cast<uint8_t *>(mem + o_mask), *d_refused = reinterpret_cast<uint8_t *>(mem + o_refused);
    frirl_hip_agent greedy = b->agent;
    greedy.no_random = 1;                                             // the teacher shows its greedy policy, as frirl_hip_batch_evaluate rolls out
    frirl_hip_rulebases one = b->rb;                                  // the teacher's slab alone: it is log 0 of a one-agent call
    one.E = 1;
    one.rb = b->rb.rb + (size_t)teacher * (ns + 2) * (size_t)b->maxR;
    one.nrules = b->rb.nrules + teacher;
    if (one.uidx) one.uidx = b->rb.uidx + (size_t)teacher * (ns + 1) * (size_t)b->maxR;
    std::vector<int32_t> h_eps(2 * K + 1), h_replayed(E);
    std::vector<uint8_t> h_refused(E);
    int rc = FRIRL_HIP_OK;
    hipError_t he = hipMemcpyAsync(d_mask, mask.data(), E, hipMemcpyHostToDevice, b->s);
    if (he == hipSuccess && start_states) {
        lg.start_states = reinterpret_cast<double *>(mem + o_st);
        he = hipMemcpyAsync(mem + o_st, start_states, sizeof(double) * K * ns, hipMemcpyHostToDevice, b->s);
    }
    if (he == hipSuccess) rc = frirl_hip_rollout_record(&b->t, &one, &greedy, &lg, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) {
        hipLaunchKernelGGL(frirl::teach_lengths_kernel, dim3((b->E + 255) / 256), dim3(256), 0, b->s, d_mask, lg.length, b->E, d_length);
        frirl_hip_demonstration dm = {};
        dm.T = lg.T; dm.agent_stride = 0;
        dm.obs = lg.obs; dm.q_obs = lg.q_obs; dm.action = lg.action; dm.reward = lg.reward; dm.success = lg.success; dm.start = lg.start; dm.length = d_length;
        rc = frirl_hip_learn_demonstration(&b->t, &b->rb, &b->agent, &b->envs, &dm, passes, d_replayed, d_refused, b->s);
    }
    if (he == hipSuccess && rc == FRIRL_HIP_OK) {
        hipLaunchKernelGGL(frirl::teach_reset_kernel, dim3(b->E), dim3(256), 0, b->s, d_mask, b->d_rb, b->d_nrules, b->maxR, b->nant, b->conv);
        he = hipMemcpyAsync(h_eps.data(), lg.ep_steps, sizeof(int32_t) * K, hipMemcpyDeviceToHost, b->s);
        if (he == hipSuccess) he = hipMemcpyAsync(h_eps.data() + K, lg.ep_success, sizeof(int32_t) * K, hipMemcpyDeviceToHost, b->s);
        if (he == hipSuccess) he = hipMemcpyAsync(h_eps.data() + 2 * K, lg.length, sizeof(int32_t), hipMemcpyDeviceToHost, b->s);
        if (he == hipSuccess) he = hipMemcpyAsync(h_replayed.data(), d_replayed, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s);
        if (he == hipSuccess) he = hipMemcpyAsync(h_refused.data(), d_refused, E, hipMemcpyDeviceToHost, b->s);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(b->s);            // also on failure of a call: `own`, `mask` and `mem` may be in use
    else (void)hipStreamSynchronize(b->s);
    (void)hipFree(mem);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(he)); return FRIRL_HIP_ELAUNCH; }
    if ((rc = check_launch(who))) return rc;
    if (result) {
        frirl_hip_teach_result out = {};
        out.teacher = teacher;
        out.records = h_eps[2 * K];
        out.students = nstudents;
        for (size_t k = 0; k < K; k++) {
            out.episodes_recorded += h_eps[k] >= 0 ? 1 : 0;
            out.successes += (h_eps[k] >= 0 && h_eps[K + k] == 1) ? 1 : 0;
        }
        for (size_t e = 0; e < E; e++) {
            if (!mask[e]) continue;
            out.refused += h_refused[e] ? 1 : 0;
            out.records_replayed += h_replayed[e];
        }
        *result = out;
    }
    return FRIRL_HIP_OK;
}

// ---- selection: clone the best agents over the worst (frirl_hip_clone_agents, clone.hip) -----------------------------------------
namespace frirl {
// inherit_rows: every set column takes the source's value for the cloned agents; in place, since a source is no destination
__global__ void inherit_rows_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ status, int E, double *d0, double *d1, double *d2, double *d3,
                                    double *d4, double *d5, int32_t *i0, int32_t *i1, uint8_t *b0, uint8_t *b1)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || status[e] != FRIRL_HIP_CLONE_CLONED) return;
    const int s = src[e];
    double *d[6] = {d0, d1, d2, d3, d4, d5};
#pragma unroll
    for (int c = 0; c < 6; c++) if (d[c]) d[c][e] = d[c][s];
    if (i0) i0[e] = i0[s];
    if (i1) i1[e] = i1[s];
    if (b0) b0[e] = b0[s];
    if (b1) b1[e] = b1[s];
}

// what one frirl_hip_batch_evolve_step reads back: the plan's info, then what the reduction below and the perturbation count
struct EvolveBlock {
    frirl_hip_select_info info;
    int32_t replaced, perturbed;
    unsigned long long rules_copied;
    int32_t best_successes, reserved;
    double best_reward;
};                                  // 48 bytes

// behind clone and perturbation: agents cloned and the rules they took over (nrules[e] is nrules[src[e]] by now), the best agent's score
__global__ __launch_bounds__(256) void evolve_reduce_kernel(const int32_t *__restrict__ status, const int32_t *__restrict__ nrules, int E,
                                                            const frirl_hip_rollout_score *__restrict__ scores, EvolveBlock *__restrict__ out)
{
    __shared__ int s_n;
    __shared__ unsigned long long s_rules;
    if (threadIdx.x == 0) { s_n = 0; s_rules = 0; }
    __syncthreads();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E && status[e] == FRIRL_HIP_CLONE_CLONED) {
        atomicAdd(&s_n, 1);
        atomicAdd(&s_rules, (unsigned long long)nrules[e]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (s_n) { atomicAdd(&out->replaced, s_n); atomicAdd(&out->rules_copied, s_rules); }
    const int best = out->info.best;
    if (blockIdx.x == 0 && best >= 0 && best < E) { out->best_successes = scores[best].successes; out->best_reward = scores[best].reward_sum; }
}
}  // namespace frirl

// frirl_hip_batch_clone(inherit_rows != 0): the gather of every set column, queued behind the clone
static void queue_inherit_rows(frirl_hip_batch *b, const int32_t *d_src, const int32_t *d_status)
{
    if (!(b->hp_set || b->ex_set || b->tq_set || b->xp_set)) return;
    const frirl_hip_hparam_rows &h = b->hp;
    hipLaunchKernelGGL(frirl::inherit_rows_kernel, dim3((b->E + 255) / 256), dim3(256), 0, b->s, d_src, d_status, b->E, const_cast<double *>(h.alpha),
                       const_cast<double *>(h.gamma), const_cast<double *>(h.qdiff_pos_boundary), const_cast<double *>(h.qdiff_neg_boundary),
                       const_cast<double *>(h.weight_significant), const_cast<double *>(b->ex.epsilon), const_cast<int32_t *>(h.skip_rules),
                       const_cast<int32_t *>(b->ex.horizon), const_cast<uint8_t *>(b->tq.target), const_cast<uint8_t *>(b->xp.expected));
}

static int batch_clone_run(const char *who, frirl_hip_batch *b, const int32_t *src, int inherit_rows, int32_t *cloned, int64_t *rules_copied)
{
    if (!b || !src) { set_error("%s: NULL batch or src", who); return FRIRL_HIP_EINVAL; }
    const int E = b->E;
    for (int e = 0; e < E; e++) {
        if (src[e] < 0 || src[e] >= E) { set_error("%s: agent %d: src=%d outside 0..%d", who, e, src[e], E - 1); return FRIRL_HIP_EINVAL; }
        if (src[src[e]] != src[e]) { set_error("%s: agent %d: its source %d is itself replaced (by %d)", who, e, src[e], src[src[e]]); return FRIRL_HIP_EINVAL; }
    }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    int32_t *d_src = nullptr;                                         // src, then status
    BCHK(hipMalloc(reinterpret_cast<void **>(&d_src), sizeof(int32_t) * 2 * (size_t)E), "clone buffers");
    int32_t *d_status = d_src + E;
    std::vector<int32_t> st(E), nr(E);
    int rc = FRIRL_HIP_OK;
    hipError_t he = hipMemcpyAsync(d_src, src, sizeof(int32_t) * E, hipMemcpyHostToDevice, b->s);
    // no image of a rule base outlives a call (d_lanes_ws and d_learn_ws are imported from rb / uidx at the start of every call that
    // uses them), so there is nothing to invalidate beside the arrays the clone itself rewrites
    if (he == hipSuccess) rc = frirl_hip_clone_agents(&b->rb, b->nant, &b->envs, &b->conv, b->d_weights, d_src, d_status, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK && inherit_rows) queue_inherit_rows(b, d_src, d_status);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemcpyAsync(st.data(), d_status, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemcpyAsync(nr.data(), b->d_nrules, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s);
    if (he == hipSuccess) he = hipStreamSynchronize(b->s);            // also on failure of the call: `src` may be in use by the upload
    else (void)hipStreamSynchronize(b->s);
    (void)hipFree(d_src);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(he)); return FRIRL_HIP_ELAUNCH; }
    if ((rc = check_launch(who))) return rc;
    int32_t count = 0;
    int64_t rules = 0;
    for (int e = 0; e < E; e++)
        if (st[e] == FRIRL_HIP_CLONE_CLONED) { count++; rules += nr[e]; }         // nrules[e] is nrules[src[e]] now
    if (cloned) *cloned = count;
    if (rules_copied) *rules_copied = rules;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_clone(frirl_hip_batch *b, const int32_t *src, int inherit_rows, int32_t *cloned)
{
    return batch_clone_run("frirl_hip_batch_clone", b, src, inherit_rows, cloned, nullptr);
}

extern "C" int frirl_hip_batch_select(frirl_hip_batch *b, int32_t n, const double *start_states, int32_t parents, int32_t replace, int inherit_rows,
                                      frirl_hip_rollout_score *scores, int32_t *src_out, frirl_hip_select_result *result)
{
    static const char *who = "frirl_hip_batch_select";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    std::vector<frirl_hip_rollout_score> sc(b->E);
    std::vector<int32_t> src(b->E);
    int32_t best = 0, cloned = 0;
    int64_t rules = 0;
    int rc = frirl_hip_batch_evaluate(b, n, start_states, sc.data(), &best);
    if (rc == FRIRL_HIP_OK) rc = frirl_hip_select_plan(sc.data(), b->E, nullptr, parents, replace, src.data(), nullptr);
    if (rc == FRIRL_HIP_OK) rc = batch_clone_run(who, b, src.data(), inherit_rows, &cloned, &rules);
    if (rc) return rc;
    if (scores) memcpy(scores, sc.data(), sizeof(frirl_hip_rollout_score) * b->E);
    if (src_out) memcpy(src_out, src.data(), sizeof(int32_t) * b->E);
    if (result) *result = frirl_hip_select_result{best, parents, cloned, 0, rules};
    return FRIRL_HIP_OK;
}

// ---- population-based training: the selection leg queued on the stream, one read-back (select_device.hip) --------------------------
// what frirl_hip_batch_evolve_step refuses before it looks at the device
static int evolve_args_check(const char *who, const frirl_hip_batch *b, int32_t n, int32_t parents, int32_t replace, const frirl_hip_perturb_spec *spec)
{
    if (evaluate_args_check(who, b, n)) return FRIRL_HIP_EINVAL;
    if (parents < 1) { set_error("%s: parents=%d < 1", who, parents); return FRIRL_HIP_EINVAL; }
    if (replace < 0) { set_error("%s: replace=%d < 0", who, replace); return FRIRL_HIP_EINVAL; }
    if ((int64_t)parents + replace > b->E) {
        set_error("%s: parents=%d + replace=%d exceeds the %d agents (a parent would be replaced)", who, parents, replace, b->E);
        return FRIRL_HIP_EINVAL;
    }
    if (!spec) return FRIRL_HIP_OK;
    if (frirl_hip_perturb_spec_check(spec)) return FRIRL_HIP_EINVAL;
    const void *set[8] = {b->hp.alpha, b->hp.gamma, b->hp.weight_significant, b->ex.epsilon, b->ex.horizon, b->hp.skip_rules, b->tq.target, b->xp.expected};
    for (int c = 0; c < 8; c++)
        if ((spec->columns >> c & 1) && !set[c]) {
            set_error("%s: the spec perturbs %s, a column this batch has not set (frirl_hip_batch_set_*)", who, frirl_hip_perturb_column_name(c));
            return FRIRL_HIP_EINVAL;
        }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_evolve_step(frirl_hip_batch *b, int32_t n, const double *start_states, int32_t parents, int32_t replace, int inherit_rows,
                                           const frirl_hip_perturb_spec *spec, frirl_hip_evolve_result *result)
{
    static const char *who = "frirl_hip_batch_evolve_step";
    if (evolve_args_check(who, b, n, parents, replace, spec)) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const int E = b->E;
    const size_t block_at = ((size_t)3 * E + 3) / 4 * 4;             // in int32s: the block starts on a 16-byte boundary
    if (!b->d_evo && !dalloc(&b->d_evo, block_at + sizeof(frirl::EvolveBlock) / sizeof(int32_t))) {
        set_error("%s: HIP allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return FRIRL_HIP_ELAUNCH;
    }
    int32_t *d_src = b->d_evo, *d_rank = d_src + E, *d_status = d_rank + E;
    frirl::EvolveBlock *d_block = reinterpret_cast<frirl::EvolveBlock *>(b->d_evo + block_at), h = {};
    EvalQueued q;
    hipError_t he = hipSuccess;
    int rc = batch_evaluate_queue(b, n, start_states, q, he);
    if (!q.mem) return rc;                                            // nothing was queued
    if (he == hipSuccess && rc == FRIRL_HIP_OK) he = hipMemsetAsync(d_block, 0, sizeof *d_block, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) rc = frirl_hip_select_plan_device(q.scores(), E, nullptr, parents, replace, d_src, d_rank, &d_block->info, b->s);
    // a plan refused on the device left src at the identity: everything behind it then finds nobody cloned
    if (he == hipSuccess && rc == FRIRL_HIP_OK) rc = frirl_hip_clone_agents(&b->rb, b->nant, &b->envs, &b->conv, b->d_weights, d_src, d_status, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK && inherit_rows) queue_inherit_rows(b, d_src, d_status);
    if (he == hipSuccess && rc == FRIRL_HIP_OK && spec)
        rc = frirl_hip_perturb_rows(spec, b->generation, E, d_status, &b->hp, &b->ex, &b->tq, &b->xp, &d_block->perturbed, b->s);
    if (he == hipSuccess && rc == FRIRL_HIP_OK) {
        hipLaunchKernelGGL(frirl::evolve_reduce_kernel, dim3((E + 255) / 256), dim3(256), 0, b->s, d_status, b->d_nrules, E, q.scores(), d_block);
        he = hipMemcpyAsync(&h, d_block, sizeof h, hipMemcpyDeviceToHost, b->s);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(b->s);            // also on failure of a call: `q.own` and `q.mem` may be in use by the upload
    else (void)hipStreamSynchronize(b->s);
    (void)hipFree(q.mem);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(he)); return FRIRL_HIP_ELAUNCH; }
    if ((rc = check_launch(who))) return rc;
    if (h.info.status == FRIRL_HIP_PLAN_NAN) { set_error("%s: agent %d: reward_sum is NaN (nothing was cloned)", who, h.info.bad_agent); return FRIRL_HIP_EINVAL; }
    if (h.info.status != FRIRL_HIP_PLAN_OK) {
        set_error("%s: plan status %d: parents=%d + replace=%d exceeds the %d eligible agents, bad_agent %d (nothing was cloned)", who, h.info.status, parents, replace,
                  h.info.N, h.info.bad_agent);
        return FRIRL_HIP_EINVAL;
    }
    if (result) *result = frirl_hip_evolve_result{h.info.best, parents, h.replaced, h.perturbed, (int64_t)h.rules_copied, (int32_t)b->generation, h.info.status};
    b->generation++;
    b->evo_scored = true; b->evo_successes = h.best_successes; b->evo_reward = h.best_reward;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_evolve_best_score(frirl_hip_batch *b, int32_t *successes, double *reward_sum)
{
    static const char *who = "frirl_hip_batch_evolve_best_score";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (!b->evo_scored) { set_error("%s: no frirl_hip_batch_evolve_step has succeeded on this batch yet", who); return FRIRL_HIP_EINVAL; }
    if (successes) *successes = b->evo_successes;
    if (reward_sum) *reward_sum = b->evo_reward;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_evolve(frirl_hip_batch *b, int32_t generations, int32_t episodes_per_generation, int32_t n, const double *start_states,
                                      int32_t parents, int32_t replace, int inherit_rows, const frirl_hip_perturb_spec *spec, frirl_hip_evolve_result *results)
{
    static const char *who = "frirl_hip_batch_evolve";
    if (!b) { set_error("%s: NULL batch", who); return FRIRL_HIP_EINVAL; }
    if (generations < 1 || episodes_per_generation < 1) {
        set_error("%s: generations=%d / episodes_per_generation=%d below 1", who, generations, episodes_per_generation);
        return FRIRL_HIP_EINVAL;
    }
    if (evolve_args_check(who, b, n, parents, replace, spec)) return FRIRL_HIP_EINVAL;      // before anything is trained
    for (int32_t g = 0; g < generations; g++) {
        int rc = frirl_hip_batch_train(b, episodes_per_generation + 1, nullptr);
        if (rc == FRIRL_HIP_OK) rc = frirl_hip_batch_evolve_step(b, n, start_states, parents, replace, inherit_rows, spec, results ? results + g : nullptr);
        if (rc) return rc;
    }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_get_hparams(frirl_hip_batch *b, const frirl_hip_hparam_rows *host_out)
{
    static const char *who = "frirl_hip_batch_get_hparams";
    if (!b || !host_out) { set_error("%s: NULL batch or host_out", who); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    BCHK(hipStreamSynchronize(b->s), "hyper-parameter sync");
    const size_t E = (size_t)b->E;
    const double *out[5] = {host_out->alpha, host_out->gamma, host_out->qdiff_pos_boundary, host_out->qdiff_neg_boundary, host_out->weight_significant};
    const double *set[5] = {b->hp.alpha, b->hp.gamma, b->hp.qdiff_pos_boundary, b->hp.qdiff_neg_boundary, b->hp.weight_significant};
    const double own[5] = {b->agent.alpha, b->agent.gamma, b->agent.qdiff_pos_boundary, b->agent.qdiff_neg_boundary, b->agent.weight_significant};
    for (int c = 0; c < 5; c++) {
        if (!out[c]) continue;
        if (set[c]) BCHK(hipMemcpy(const_cast<double *>(out[c]), set[c], sizeof(double) * E, hipMemcpyDeviceToHost), "hyper-parameter download");
        else std::fill_n(const_cast<double *>(out[c]), E, own[c]);
    }
    if (host_out->skip_rules) {
        if (b->hp.skip_rules) BCHK(hipMemcpy(const_cast<int32_t *>(host_out->skip_rules), b->hp.skip_rules, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "hyper-parameter download");
        else std::fill_n(const_cast<int32_t *>(host_out->skip_rules), E, (int32_t)b->agent.skip_rules);
    }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_get_exploration(frirl_hip_batch *b, const frirl_hip_explore_rows *host_out)
{
    static const char *who = "frirl_hip_batch_get_exploration";
    if (!b || !host_out) { set_error("%s: NULL batch or host_out", who); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    BCHK(hipStreamSynchronize(b->s), "exploration sync");
    const size_t E = (size_t)b->E;
    if (host_out->epsilon) {
        if (b->ex.epsilon) BCHK(hipMemcpy(const_cast<double *>(host_out->epsilon), b->ex.epsilon, sizeof(double) * E, hipMemcpyDeviceToHost), "exploration download");
        else std::fill_n(const_cast<double *>(host_out->epsilon), E, b->agent.epsilon);
    }
    if (host_out->horizon) {
        if (b->ex.horizon) BCHK(hipMemcpy(const_cast<int32_t *>(host_out->horizon), b->ex.horizon, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "exploration download");
        else std::fill_n(const_cast<int32_t *>(host_out->horizon), E, b->ex.horizon_all);
    }
    return FRIRL_HIP_OK;
}

// ---- multi-agent rule-base merge: one round of the reference's many-agent loop (frirl_agent.c:426-462) -------------------
// (1) every agent id >= 1 takes over the master's (agent 0's) rules -- all receivers in ONE launch; (2) the master takes over the
// rules of agent 1, 2, ... one after the other (sequential by definition: each merge changes the master).  Agents whose rule base
// passed the cheap completeness test in this chunk (`epended`) do not send, as in the reference (frirl_agent.c:338,352).
// ---- the pieces of a merge round (batch_internal.h; also strung together across devices by multi.hip) --------------------------
namespace frirl_host {

BatchView batch_view(frirl_hip_batch *b)
{
    return BatchView{b->nant, b->maxR, b->E, b->device, b->s, b->d_rant, b->d_rb, b->d_nrules, b->d_converged, b->d_epended};
}

int batch_merge_prepare(frirl_hip_batch *b, std::vector<int32_t> &pended)
{
    std::vector<int32_t> &conv = pended;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t M = b->maxR, E = b->E;
    if (!b->d_weights) {
        if (!dalloc(&b->d_weights, E * M) || !dalloc(&b->d_active, E) || !dalloc(&b->d_full, E)) { set_error("frirl_hip_batch_merge_round: allocation failed"); return FRIRL_HIP_ELAUNCH; }
    }
    conv.resize(E);
    BCHK(hipMemcpyAsync(conv.data(), b->d_epended, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s), "epended download");
    BCHK(hipStreamSynchronize(b->s), "merge sync");
    // the receivers' FIVERB.weights as the learning episodes left them (the reference's merge starts from that array)
    return frirl_hip_weights_from_spread(&b->t, &b->rb, b->agent.p, &b->envs, b->d_weights, b->s);
}

int batch_merge_into_agents(frirl_hip_batch *b, const frirl_hip_sender *snd, bool skip_first)
{
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t E = b->E;
    if (skip_first && E < 2) return FRIRL_HIP_OK;
    std::vector<uint8_t> act(E, 1);
    if (skip_first) act[0] = 0;
    BCHK(hipMemcpyAsync(b->d_active, act.data(), E, hipMemcpyHostToDevice, b->s), "active upload");
    const int rc = frirl_hip_merge_rb(&b->t, &b->rb, &b->agent, b->d_rant, snd, b->d_weights, b->d_active, b->d_full, b->s);
    if (rc) return rc;
    BCHK(hipStreamSynchronize(b->s), "merge sync");              // `act` must outlive the upload
    return FRIRL_HIP_OK;
}

int batch_merge_into_first(frirl_hip_batch *b, const frirl_hip_sender *snd)
{
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    frirl_hip_rulebases master = b->rb;
    master.E = 1;
    return frirl_hip_merge_rb(&b->t, &master, &b->agent, b->d_rant, snd, b->d_weights, nullptr, b->d_full, b->s);
}

frirl_hip_sender batch_sender(frirl_hip_batch *b, int id)
{
    const size_t n = b->nant, M = b->maxR;
    frirl_hip_sender snd;
    memset(&snd, 0, sizeof snd);
    snd.rule_stride = 1; snd.dim_stride = (int64_t)M;
    snd.rant = b->d_rant + (size_t)id * n * M;
    snd.rconc = b->d_rb + ((size_t)id * (n + 1) + n) * M;
    snd.S_dev = b->d_nrules + id;
    return snd;
}

int batch_merge_finish(frirl_hip_batch *b, int32_t *full_agents, bool first_is_master)
{
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t E = b->E;
    b->h_i.resize(E);
    BCHK(hipMemcpyAsync(b->h_i.data(), b->d_nrules, sizeof(int32_t) * E, hipMemcpyDeviceToHost, b->s), "nrules download");
    BCHK(hipStreamSynchronize(b->s), "merge sync");
    if (full_agents) for (size_t e = 0; e < E; e++) *full_agents += b->h_i[e] >= b->maxR;
    hipLaunchKernelGGL(frirl::next_round_kernel, dim3((b->E + 255) / 256), dim3(256), 0, b->s, b->d_converged, b->d_epended, b->E, first_is_master ? 1 : 0);
    // rule count and consequents of the next convergence test are retaken from the merged rule bases (frirl_sequential_run.c:66-72)
    const int rc = frirl_hip_convergence_refresh(&b->rb, b->nant, &b->conv, b->s);
    if (rc) return rc;
    BCHK(hipStreamSynchronize(b->s), "merge sync");
    return FRIRL_HIP_OK;
}

}  // namespace frirl_host

extern "C" int frirl_hip_batch_merge_round(frirl_hip_batch *b, int32_t *full_agents)
{
    if (!b) { set_error("frirl_hip_batch_merge_round: NULL batch"); return FRIRL_HIP_EINVAL; }
    if (refuse_rows(b, "frirl_hip_batch_merge_round")) return FRIRL_HIP_EINVAL;
    if (full_agents) *full_agents = 0;
    if (b->E < 2) return FRIRL_HIP_OK;
    std::vector<int32_t> conv;
    int rc = batch_merge_prepare(b, conv);
    if (rc) return rc;
    if (!conv[0]) {                                                   // (1) master -> every other agent
        const frirl_hip_sender snd = batch_sender(b, 0);
        if ((rc = batch_merge_into_agents(b, &snd, true))) return rc;
    }
    for (int id = 1; id < b->E; id++) {                               // (2) agent id -> master, id ascending
        if (conv[id]) continue;
        const frirl_hip_sender snd = batch_sender(b, id);
        if ((rc = batch_merge_into_first(b, &snd))) return rc;
    }
    return batch_merge_finish(b, full_agents, true);
}

// frirl_omp_run's loop (frirl_agent.c:319-360) for the agents of this batch: every round each agent runs a chunk of at most
// `chunk - 1` episodes (FRIRL_AGENT_EPCHUNK = 10 in the reference's config.h.in:68; an agent whose rule base is found complete stops
// for the rest of ITS chunk and runs again in the next round), then one exchange round gated by that chunk's `epended` flags -- until
// the master's rule base is complete or the master has started max_episodes episodes, which frirl_sequential_run only looks at when a
// chunk is over (:57-63): the master always finishes its chunk.  *episodes_run = the master's episodes.
extern "C" int frirl_hip_batch_train_merged(frirl_hip_batch *b, int32_t max_episodes, int32_t chunk, int32_t *episodes_run, int32_t *rounds)
{
    if (!b || chunk < 2) { set_error("frirl_hip_batch_train_merged: bad arguments"); return FRIRL_HIP_EINVAL; }
    if (refuse_rows(b, "frirl_hip_batch_train_merged")) return FRIRL_HIP_EINVAL;
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    int episode_num = 1, episodes = 0, nrounds = 0;         // frirl_desc.episode_num of the master starts at 1 (frirl_init.c)
    for (;;) {
        int32_t master_done = 0;
        for (int c = 1; c < chunk; c++) {
            const int rc = frirl_hip_batch_episode(b);
            if (rc) return rc;
            episodes++;
            BCHK(hipMemcpy(&master_done, b->d_converged, sizeof(int32_t), hipMemcpyDeviceToHost), "converged download");
            if (master_done) break;
            episode_num++;
        }
        if (master_done || !(episode_num < max_episodes)) break;
        const int rc = frirl_hip_batch_merge_round(b, nullptr);
        if (rc) return rc;
        nrounds++;
    }
    if (episodes_run) *episodes_run = episodes;
    if (rounds) *rounds = nrounds;
    return FRIRL_HIP_OK;
}

// ---- batched rule-base I/O in the reference's .frirlrb.bin record format (frirl_utils.c:151-281) ------------------------
extern "C" int frirl_hip_batch_save_rulebases(frirl_hip_batch *b, const char *path)
{
    if (!b || !path) { set_error("frirl_hip_batch_save_rulebases: bad arguments"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t n = b->nant, M = b->maxR, E = b->E;
    std::vector<int32_t> nr(E);
    std::vector<double> rant(E * n * M), rb(E * (n + 1) * M);
    BCHK(hipStreamSynchronize(b->s), "save sync");
    BCHK(hipMemcpy(nr.data(), b->d_nrules, sizeof(int32_t) * E, hipMemcpyDeviceToHost), "nrules download");
    BCHK(hipMemcpy(rant.data(), b->d_rant, sizeof(double) * rant.size(), hipMemcpyDeviceToHost), "rant download");
    BCHK(hipMemcpy(rb.data(), b->d_rb, sizeof(double) * rb.size(), hipMemcpyDeviceToHost), "rb download");
    FILE *fp = fopen(path, "wb");
    if (!fp) { set_error("frirl_hip_batch_save_rulebases: cannot open %s", path); return FRIRL_HIP_EINVAL; }
    std::vector<double> rec;
    bool ok = true;
    for (size_t e = 0; e < E && ok; e++) {
        const int32_t R = nr[e];
        rec.resize((size_t)R * (n + 1));
        for (int r = 0; r < R; r++) {
            for (size_t k = 0; k < n; k++) rec[(size_t)r * (n + 1) + k] = rant[(e * n + k) * M + r];
            rec[(size_t)r * (n + 1) + n] = rb[(e * (n + 1) + n) * M + r];
        }
        ok = fwrite(&R, sizeof R, 1, fp) == 1 && (R == 0 || fwrite(rec.data(), sizeof(double), rec.size(), fp) == rec.size());
    }
    ok = (fclose(fp) == 0) && ok;
    if (!ok) { set_error("frirl_hip_batch_save_rulebases: write to %s failed", path); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_load_rulebases(frirl_hip_batch *b, const char *path, int32_t *records_read)
{
    if (!b || !path) { set_error("frirl_hip_batch_load_rulebases: bad arguments"); return FRIRL_HIP_EINVAL; }
    DeviceGuard keep_device_; BCHK(hipSetDevice(b->device), "hipSetDevice");
    const size_t n = b->nant, M = b->maxR, E = b->E;
    FILE *fp = fopen(path, "rb");
    if (!fp) { set_error("frirl_hip_batch_load_rulebases: cannot open %s", path); return FRIRL_HIP_EINVAL; }
    // parse and validate the whole file before touching the batch
    std::vector<std::vector<double>> recs;
    for (;;) {
        int32_t R = 0;
        const size_t got = fread(&R, 1, sizeof R, fp);
        if (got == 0) break;                                   // clean end of file
        if (got != sizeof R) { fclose(fp); set_error("frirl_hip_batch_load_rulebases: %s: truncated record header", path); return FRIRL_HIP_EINVAL; }
        if (R < 1 || (size_t)R > M) { fclose(fp); set_error("frirl_hip_batch_load_rulebases: %s: record %zu has %d rules (capacity %zu)", path, recs.size(), R, M); return FRIRL_HIP_EINVAL; }
        std::vector<double> rec((size_t)R * (n + 1));
        if (fread(rec.data(), sizeof(double), rec.size(), fp) != rec.size()) { fclose(fp); set_error("frirl_hip_batch_load_rulebases: %s: record %zu is truncated", path, recs.size()); return FRIRL_HIP_EINVAL; }
        for (double v : rec) if (!(v - v == 0.0)) { fclose(fp); set_error("frirl_hip_batch_load_rulebases: %s: record %zu holds a non-finite value", path, recs.size()); return FRIRL_HIP_EINVAL; }
        recs.push_back(std::move(rec));
        if (recs.size() == E) break;
    }
    fclose(fp);
    if (recs.empty()) { set_error("frirl_hip_batch_load_rulebases: %s holds no rule base", path); return FRIRL_HIP_EINVAL; }
    if (records_read) *records_read = (int32_t)recs.size();
    // rebuild: nrules = 0, then rule r of every agent through FIVE_add_rule (agents whose record is shorter sit out)
    BCHK(hipMemsetAsync(b->d_nrules, 0, sizeof(int32_t) * E, b->s), "nrules reset");
    BCHK(hipMemsetAsync(b->d_fus, 0, sizeof(int32_t) * E, b->s), "fus reset");            // frirl_utils.c:262
    size_t rmax = 0;
    for (size_t e = 0; e < E; e++) { const auto &rec = recs[e < recs.size() ? e : recs.size() - 1]; rmax = std::max(rmax, rec.size() / (n + 1)); }
    std::vector<double> stage(E * (n + 1));
    std::vector<uint8_t> act(E);
    uint8_t *d_act = nullptr;
    BCHK(hipMalloc((void **)&d_act, E), "active mask");
    int rc = FRIRL_HIP_OK;
    for (size_t r = 0; r < rmax && rc == FRIRL_HIP_OK; r++) {
        for (size_t e = 0; e < E; e++) {
            const auto &rec = recs[e < recs.size() ? e : recs.size() - 1];
            const bool has = r < rec.size() / (n + 1);
            act[e] = has ? 1 : 0;
            for (size_t k = 0; k < n; k++) stage[e * n + k] = has ? rec[r * (n + 1) + k] : 0.0;
            stage[E * n + e] = has ? rec[r * (n + 1) + n] : 0.0;
        }
        if (hipMemcpyAsync(b->d_tmp, stage.data(), sizeof(double) * E * (n + 1), hipMemcpyHostToDevice, b->s) != hipSuccess ||
            hipMemcpyAsync(d_act, act.data(), E, hipMemcpyHostToDevice, b->s) != hipSuccess) { set_error("frirl_hip_batch_load_rulebases: upload failed"); rc = FRIRL_HIP_ELAUNCH; break; }
        rc = five_hip_add_rule(&b->t, &b->rb, b->d_tmp, b->d_tmp + E * n, d_act, b->d_rant, nullptr, b->s);
        if (rc == FRIRL_HIP_OK && hipStreamSynchronize(b->s) != hipSuccess) { set_error("frirl_hip_batch_load_rulebases: add_rule failed"); rc = FRIRL_HIP_ELAUNCH; }
    }
    (void)hipFree(d_act);
    if (rc) return rc;
    if ((rc = frirl_hip_convergence_init(&b->rb, b->nant, &b->conv, b->s))) return rc;
    BCHK(hipStreamSynchronize(b->s), "load sync");
    return FRIRL_HIP_OK;
}
