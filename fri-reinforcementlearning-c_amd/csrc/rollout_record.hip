// rollout_record.hip -- frirl_hip_rollout_record (include/frirl_hip.h, DESIGN.md "Recorded roll-outs"): the greedy (or epsilon-greedy)
// roll-outs of frirl_hip_rollout_batch's tiled form with EVERY step written out, in the layout frirl_hip_learn_demonstration reads:
// E * n logs of K episodes each, log q = e * n + j on the slab of agent e = q / n.
//
// Launches of a call, nothing read back in between:
//   prep     the logs that are not recorded (j >= row_count[e], an inactive agent, nrules[e] outside 1..maxR) get length 0 and
//            ep_steps -1 / ep_reward 0 / ep_success 0 for every episode
//   record   a workgroup serves logs of ONE agent through rollout_record_episodes / shared_sweep (the LDS rule tiles are shared); which
//            logs exist is decided again by the same comparison on the device
#include "rollout_record_episodes.h"
#include "batch_shape.h"
#include "shape_ladder.h"

namespace frirl {

// logs of agent e that are recorded.  The descriptor goes by reference on purpose: the record kernel's registers depend on it
// (profiles/r24_rollout_loop.md, section 3).
__device__ __forceinline__ int record_rows(const frirl_hip_rollout_log &lg, const int32_t *__restrict__ nrules, int maxR, int e)
{
    return agent_rows(lg.row_count, lg.active, lg.n, nrules, maxR, e);
}

__global__ __launch_bounds__(256) void rollout_record_prep_kernel(const int32_t *__restrict__ nrules, int E, int maxR, const frirl_hip_rollout_log lg)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)E * lg.n) return;
    const int e = (int)(q / lg.n), j = (int)(q - (long)e * lg.n);
    if (j < record_rows(lg, nrules, maxR, e)) return;
    lg.length[q] = 0;
    for (int k = 0; k < lg.episodes; k++) {
        const size_t i = (size_t)q * lg.episodes + k;
        if (lg.ep_steps) lg.ep_steps[i] = -1;
        if (lg.ep_reward) lg.ep_reward[i] = 0.0;
        if (lg.ep_success) lg.ep_success[i] = 0;
    }
}

// `wpa` workgroups per agent, each serving 256 / (G * H) logs of that agent.  All conditions in front of the barriers are uniform over
// the workgroup: they depend on the agent and on the workgroup's first log only.
template <int NANT, int AMAX, int G, int H, bool PN>
__global__ __launch_bounds__(SH_BLOCK) void rollout_record_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                                   const double *__restrict__ rb, const int32_t *__restrict__ nrules, int maxR,
                                                                   const frirl_hip_agent ag, int wpa, const frirl_hip_rollout_log lg)
{
    constexpr int GH = G * H, EPB = SH_BLOCK / GH;
    __shared__ SharedTile<NANT> tl;
    __shared__ double grid_s[NANT * FRIRL_HIP_MAX_GRID];
    const int e = (int)(blockIdx.x / (unsigned)wpa);
    const int row0 = (int)(blockIdx.x % (unsigned)wpa) * EPB;
    const int rows = record_rows(lg, nrules, maxR, e);
    if (row0 >= rows) return;                                         // nothing to record here
    const int j = row0 + threadIdx.x / GH;
    const bool exists = j < rows;
    const size_t q = (size_t)e * lg.n + (exists ? j : 0);
    using POW = KernelPow<NANT, PN>;
    const POW p = kernel_pow<NANT, PN>(ag);
    rollout_record_episodes<NANT, AMAX, G, H, POW>(tl, grid_s, u, ve, U, rb + (size_t)e * (NANT + 1) * maxR, nrules[e], maxR, ag, p, exists, q, lg);
}

}  // namespace frirl

using namespace frirl_host;

namespace {

template <int N, int AMAX, int G, int H, bool PN>
void launch_record(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_log *lg, hipStream_t s)
{
    constexpr int EPB = frirl::SH_BLOCK / (G * H);
    const int wpa = (lg->n + EPB - 1) / EPB;
    hipLaunchKernelGGL((frirl::rollout_record_kernel<N, AMAX, G, H, PN>), dim3((unsigned)b->E * (unsigned)wpa), dim3(frirl::SH_BLOCK), 0, s, t->u, t->ve,
                       t->U, b->rb, b->nrules, b->maxR, *ag, wpa, *lg);
}

template <int N>
void launch_record_n(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_rollout_log *lg, hipStream_t s)
{
    frirl::for_batch_shape<N>(ag, rb_rollout_slices(b->E, lg->n, ag->A, opts().rollout_record_slices), [&](auto sh) {
        using S = decltype(sh);
        launch_record<N, S::AMAX, S::G, S::H, S::PN>(t, b, ag, lg, s);
    });
}

}  // namespace

extern "C" int frirl_hip_rollout_record(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                        const frirl_hip_rollout_log *log, void *stream)
{
    static const char *who = "frirl_hip_rollout_record";
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if ((rc = check_rollout_agent_null(agent, log != nullptr, who))) return rc;
    if (!log->obs || !log->action || !log->reward || !log->success || !log->start || !log->length) {
        set_error("%s: NULL obs / action / reward / success / start / length", who);
        return FRIRL_HIP_EINVAL;
    }
    if (log->n < 1) { set_error("%s: n=%d < 1", who, log->n); return FRIRL_HIP_EINVAL; }
    if (log->episodes < 1) { set_error("%s: episodes=%d < 1", who, log->episodes); return FRIRL_HIP_EINVAL; }
    if (log->T < 2) { set_error("%s: T=%d < 2", who, log->T); return FRIRL_HIP_EINVAL; }
    if ((int64_t)b->E * log->n > INT32_MAX) { set_error("%s: E * n = %lld logs exceed INT32_MAX", who, (long long)b->E * log->n); return FRIRL_HIP_EINVAL; }
    int64_t records = 0, episodes = 0;
    if (__builtin_mul_overflow((int64_t)b->E * log->n, (int64_t)log->T, &records) || __builtin_mul_overflow((int64_t)b->E * log->n, (int64_t)log->episodes, &episodes)) {
        set_error("%s: E * n * T overflows int64", who);
        return FRIRL_HIP_EINVAL;
    }
    if ((rc = check_rollout_agent(t, agent, who)) || (rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    const long Q = (long)b->E * log->n;
    hipLaunchKernelGGL(frirl::rollout_record_prep_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, b->nrules, b->E, b->maxR, *log);
    if (t->nant == 3) launch_record_n<3>(t, b, agent, log, s);
    else launch_record_n<5>(t, b, agent, log, s);
    return check_launch(who);
}
