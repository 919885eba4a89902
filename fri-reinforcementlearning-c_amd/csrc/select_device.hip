// select_device.hip -- the selection leg of population-based training without the host (include/frirl_hip.h, "population-based training"):
//   frirl_hip_select_plan_device  frirl_hip_select_plan with every array on the device: rank the eligible agents, fill the src table
//   frirl_hip_perturb_rows        multiplicative steps / flips of the row values the freshly cloned agents inherited
//
// The ranking is a counting rank: the order (most successes, largest reward_sum, lowest index) is total once NaN is excluded, so the
// number of eligible agents that beat agent e IS its place, the places are a permutation of 0..N-1 and the scatter rank[place] = e
// has neither a race nor a wait between workgroups.  Four launches on the stream, each complete before the next starts:
//   plan_init_kernel    rank = -1, src = identity, info = {0, OK, -1, -1}
//   plan_count_kernel   N (one atomicAdd per workgroup) and the lowest eligible NaN agent (atomicMin on the unsigned image: -1 is the top)
//   plan_rank_kernel    a workgroup owns 64 agents; it streams all E keys through LDS in tiles of 256, wave w of the workgroup counting
//                       against quarter w of every tile (every LDS read is a broadcast), the four partial counts meet in LDS
//   plan_finish_kernel  src[rank[N-1-k]] = rank[k % parents] for k < replace; status and best into info
// A refusal decided on the device (NAN, TOO_FEW) is seen by the last two kernels in info->N / info->bad_agent, which no kernel that
// reads them writes: they then leave rank at -1 and src at the identity.
#include <math.h>

#include <algorithm>

#include "device_common.h"
#include "envs.h"

using namespace frirl_host;

namespace frirl {

constexpr int PLAN_TILE = 256;      // keys per LDS tile = threads per workgroup
constexpr int PLAN_OWN = 64;        // agents a workgroup ranks: one per lane, the same in each of its four waves

__device__ __forceinline__ bool plan_eligible(const uint8_t *__restrict__ eligible, int e) { return !eligible || eligible[e] != 0; }

// what the device alone can refuse, from the two words the count kernel leaves
__device__ __forceinline__ int plan_status(int N, int bad_agent, int parents, int replace)
{
    if (bad_agent >= 0) return FRIRL_HIP_PLAN_NAN;
    return (int64_t)parents + replace > N ? FRIRL_HIP_PLAN_TOO_FEW : FRIRL_HIP_PLAN_OK;
}

__global__ __launch_bounds__(256) void plan_init_kernel(int E, int32_t *__restrict__ src, int32_t *__restrict__ rank, frirl_hip_select_info *__restrict__ info)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) { src[e] = e; rank[e] = -1; }
    if (e == 0) { info->N = 0; info->status = FRIRL_HIP_PLAN_OK; info->best = -1; info->bad_agent = -1; }
}

__global__ __launch_bounds__(256) void plan_count_kernel(const frirl_hip_rollout_score *__restrict__ scores, int E, const uint8_t *__restrict__ eligible,
                                                         frirl_hip_select_info *__restrict__ info)
{
    __shared__ int s_n;
    __shared__ unsigned s_bad;
    if (threadIdx.x == 0) { s_n = 0; s_bad = 0xFFFFFFFFu; }
    __syncthreads();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E && plan_eligible(eligible, e)) {
        atomicAdd(&s_n, 1);
        const double r = scores[e].reward_sum;
        if (r != r) atomicMin(&s_bad, (unsigned)e);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_n) atomicAdd(&info->N, s_n);
        if (s_bad != 0xFFFFFFFFu) atomicMin(reinterpret_cast<unsigned *>(&info->bad_agent), s_bad);
    }
}

// key j beats key i: more successes, then the larger reward_sum compared as doubles (-0.0 == +0.0), then the lower index.  An
// ineligible key is stored as (INT32_MIN, NaN): it is never greater and never equal, so it beats nobody.
__device__ __forceinline__ int plan_beats(int sj, double rj, int j, int si, double ri, int i)
{
    return (sj > si) | ((sj == si) & ((rj > ri) | ((rj == ri) & (j < i))));
}

__global__ __launch_bounds__(256) void plan_rank_kernel(const frirl_hip_rollout_score *__restrict__ scores, int E, const uint8_t *__restrict__ eligible,
                                                        int parents, int replace, int32_t *__restrict__ rank, const frirl_hip_select_info *__restrict__ info)
{
    __shared__ double s_r[PLAN_TILE];
    __shared__ int s_s[PLAN_TILE];
    __shared__ int s_count[PLAN_TILE];
    const int N = info->N;
    if (plan_status(N, info->bad_agent, parents, replace) != FRIRL_HIP_PLAN_OK) return;      // uniform over the grid
    const int lane = threadIdx.x & (PLAN_OWN - 1), part = threadIdx.x / PLAN_OWN;
    const int i = blockIdx.x * PLAN_OWN + lane;
    const bool mine = i < E && plan_eligible(eligible, i);
    const int si = mine ? scores[i].successes : 0;
    const double ri = mine ? scores[i].reward_sum : 0.0;
    int count = 0;
    // the key this thread brings into the next tile is loaded while the current tile is counted
    auto key = [&](int j, int *s, double *r) {
        const bool has = j < E && plan_eligible(eligible, j);
        *s = has ? scores[j].successes : INT32_MIN;
        *r = has ? scores[j].reward_sum : __builtin_nan("");
    };
    int s_next;
    double r_next;
    key((int)threadIdx.x, &s_next, &r_next);
    for (int base = 0; base < E; base += PLAN_TILE) {
        s_s[threadIdx.x] = s_next;
        s_r[threadIdx.x] = r_next;
        __syncthreads();
        if (base + PLAN_TILE < E) key(base + PLAN_TILE + (int)threadIdx.x, &s_next, &r_next);
        const int q0 = part * PLAN_OWN;
#pragma unroll 16
        for (int q = 0; q < PLAN_OWN; q++) count += plan_beats(s_s[q0 + q], s_r[q0 + q], base + q0 + q, si, ri, i);
        __syncthreads();
    }
    s_count[threadIdx.x] = count;
    __syncthreads();
    if (part == 0 && mine) {
        const int pos = s_count[lane] + s_count[lane + PLAN_OWN] + s_count[lane + 2 * PLAN_OWN] + s_count[lane + 3 * PLAN_OWN];
        if (pos < N) rank[pos] = i;
    }
}

__global__ __launch_bounds__(256) void plan_finish_kernel(int E, int parents, int replace, int32_t *__restrict__ src, const int32_t *__restrict__ rank,
                                                          frirl_hip_select_info *__restrict__ info)
{
    const int N = info->N;
    const int st = plan_status(N, info->bad_agent, parents, replace);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) { info->status = st; info->best = (st == FRIRL_HIP_PLAN_OK && N > 0) ? rank[0] : -1; }
    if (st != FRIRL_HIP_PLAN_OK || k >= replace) return;
    const int loser = rank[N - 1 - k], parent = rank[k % parents];          // parents + replace <= N <= E: both inside rank[0..N-1]
    if (loser >= 0 && loser < E && parent >= 0 && parent < E) src[loser] = parent;
}

struct PerturbArgs {
    frirl_hip_perturb_spec spec;
    double *d[4];                   // alpha, gamma, weight_significant, epsilon: NULL = not perturbed
    int32_t *horizon, *skip_rules;
    uint8_t *target, *expected;
    const int32_t *status;
    int32_t *perturbed;
    uint32_t generation;
    int32_t E;
};

__global__ __launch_bounds__(256) void perturb_rows_kernel(const PerturbArgs a)
{
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < a.E && a.status[e] == FRIRL_HIP_CLONE_CLONED) {
        const frirl_hip_perturb_spec &sp = a.spec;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (!a.d[c]) continue;
            const double f = rng_unit(sp.seed, (uint64_t)e, a.generation, (uint32_t)c, 0) < 0.5 ? sp.down[c] : sp.up[c];
            a.d[c][e] = fmin(fmax(a.d[c][e] * f, sp.lo[c]), sp.hi[c]);
        }
        if (a.horizon) {
            const int c = FRIRL_HIP_PERTURB_HORIZON;
            const double f = rng_unit(sp.seed, (uint64_t)e, a.generation, (uint32_t)c, 0) < 0.5 ? sp.down[c] : sp.up[c];
            const double x = floor((double)a.horizon[e] * f + 0.5);
            a.horizon[e] = (int32_t)fmin(fmax(x, sp.lo[c]), sp.hi[c]);
        }
        if (a.skip_rules && rng_unit(sp.seed, (uint64_t)e, a.generation, FRIRL_HIP_PERTURB_SKIP_RULES, 0) < sp.flip[0]) a.skip_rules[e] = 1 - a.skip_rules[e];
        if (a.target && rng_unit(sp.seed, (uint64_t)e, a.generation, FRIRL_HIP_PERTURB_TARGET, 0) < sp.flip[1]) a.target[e] = (uint8_t)(1 - a.target[e]);
        if (a.expected && rng_unit(sp.seed, (uint64_t)e, a.generation, FRIRL_HIP_PERTURB_EXPECTED, 0) < sp.flip[2]) a.expected[e] = (uint8_t)(1 - a.expected[e]);
        if (a.perturbed) atomicAdd(&s_n, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(a.perturbed, s_n);
}

}  // namespace frirl

extern "C" int frirl_hip_select_plan_device(const frirl_hip_rollout_score *scores, int32_t E, const uint8_t *eligible, int32_t parents, int32_t replace,
                                            int32_t *src, int32_t *rank, frirl_hip_select_info *info, void *stream)
{
    static const char *who = "frirl_hip_select_plan_device";
    if (!scores || !src || !rank || !info) { set_error("%s: NULL scores, src, rank or info", who); return FRIRL_HIP_EINVAL; }
    if (E < 1) { set_error("%s: E=%d < 1", who, E); return FRIRL_HIP_EINVAL; }
    if (parents < 1) { set_error("%s: parents=%d < 1", who, parents); return FRIRL_HIP_EINVAL; }
    if (replace < 0) { set_error("%s: replace=%d < 0", who, replace); return FRIRL_HIP_EINVAL; }
    if ((int64_t)parents + replace > E) {
        set_error("%s: parents=%d + replace=%d exceeds the %d agents (a parent would be replaced)", who, parents, replace, E);
        return FRIRL_HIP_EINVAL;
    }
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    const unsigned per_agent = (unsigned)((E + 255) / 256);
    hipLaunchKernelGGL(frirl::plan_init_kernel, dim3(per_agent), dim3(256), 0, s, E, src, rank, info);
    hipLaunchKernelGGL(frirl::plan_count_kernel, dim3(per_agent), dim3(256), 0, s, scores, E, eligible, info);
    hipLaunchKernelGGL(frirl::plan_rank_kernel, dim3((unsigned)((E + frirl::PLAN_OWN - 1) / frirl::PLAN_OWN)), dim3(256), 0, s, scores, E, eligible, parents, replace,
                       rank, info);
    hipLaunchKernelGGL(frirl::plan_finish_kernel, dim3((unsigned)((std::max(replace, 1) + 255) / 256)), dim3(256), 0, s, E, parents, replace, src, rank, info);
    return check_launch(who);
}

static const char *const perturb_names[8] = {"alpha", "gamma", "weight_significant", "epsilon", "horizon", "skip_rules", "target", "expected"};

extern "C" const char *frirl_hip_perturb_column_name(int32_t column) { return column >= 0 && column < 8 ? perturb_names[column] : nullptr; }

extern "C" int frirl_hip_perturb_spec_check(const frirl_hip_perturb_spec *spec)
{
    static const char *who = "frirl_hip_perturb_spec_check";
    if (!spec) { set_error("%s: NULL spec", who); return FRIRL_HIP_EINVAL; }
    if (spec->reserved != 0) { set_error("%s: reserved is %u, not 0", who, spec->reserved); return FRIRL_HIP_EINVAL; }
    if (spec->columns >= 256) { set_error("%s: columns=0x%x names a column beyond 7 (expected)", who, spec->columns); return FRIRL_HIP_EINVAL; }
    auto finite = [](double v) { return v - v == 0.0; };
    for (int c = 0; c < 8; c++) {
        if (!(spec->columns >> c & 1)) continue;
        const char *name = perturb_names[c];
        if (c >= 5) {
            const double p = spec->flip[c - 5];
            if (!(p >= 0.0 && p <= 1.0)) { set_error("%s: %s: flip %g is not in [0, 1]", who, name, p); return FRIRL_HIP_EINVAL; }
            continue;
        }
        const double dn = spec->down[c], up = spec->up[c], lo = spec->lo[c], hi = spec->hi[c];
        if (!(dn >= 1.0 / 16 && dn <= 16.0)) { set_error("%s: %s: down %g is not in [1/16, 16]", who, name, dn); return FRIRL_HIP_EINVAL; }
        if (!(up >= 1.0 / 16 && up <= 16.0)) { set_error("%s: %s: up %g is not in [1/16, 16]", who, name, up); return FRIRL_HIP_EINVAL; }
        if (!finite(lo) || !finite(hi) || !(lo <= hi)) { set_error("%s: %s: bounds [%g, %g] are not finite with lo <= hi", who, name, lo, hi); return FRIRL_HIP_EINVAL; }
        if (c == FRIRL_HIP_PERTURB_EPSILON && !(lo >= 0.0 && hi <= 1.0)) { set_error("%s: %s: bounds [%g, %g] leave [0, 1]", who, name, lo, hi); return FRIRL_HIP_EINVAL; }
        if (c == FRIRL_HIP_PERTURB_WEIGHT_SIGNIFICANT && !(lo >= 0.0)) { set_error("%s: %s: lo %g is negative", who, name, lo); return FRIRL_HIP_EINVAL; }
        if (c == FRIRL_HIP_PERTURB_HORIZON && !(lo >= 0.0 && hi <= 1073741824.0)) { set_error("%s: %s: bounds [%g, %g] leave 0..2^30", who, name, lo, hi); return FRIRL_HIP_EINVAL; }
    }
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_perturb_rows(const frirl_hip_perturb_spec *spec, uint32_t generation, int32_t E, const int32_t *status, const frirl_hip_hparam_rows *hp,
                                      const frirl_hip_explore_rows *ex, const frirl_hip_target_rows *tq, const frirl_hip_expect_rows *xp, int32_t *perturbed,
                                      void *stream)
{
    static const char *who = "frirl_hip_perturb_rows";
    if (!spec || !status) { set_error("%s: NULL spec or status", who); return FRIRL_HIP_EINVAL; }
    if (E < 1) { set_error("%s: E=%d < 1", who, E); return FRIRL_HIP_EINVAL; }
    if (frirl_hip_perturb_spec_check(spec)) return FRIRL_HIP_EINVAL;
    const int rc = check_device();
    if (rc) return rc;
    auto on = [&](int c) { return (spec->columns >> c & 1) != 0; };
    frirl::PerturbArgs a = {};
    a.spec = *spec;
    a.d[0] = on(FRIRL_HIP_PERTURB_ALPHA) && hp ? const_cast<double *>(hp->alpha) : nullptr;
    a.d[1] = on(FRIRL_HIP_PERTURB_GAMMA) && hp ? const_cast<double *>(hp->gamma) : nullptr;
    a.d[2] = on(FRIRL_HIP_PERTURB_WEIGHT_SIGNIFICANT) && hp ? const_cast<double *>(hp->weight_significant) : nullptr;
    a.d[3] = on(FRIRL_HIP_PERTURB_EPSILON) && ex ? const_cast<double *>(ex->epsilon) : nullptr;
    a.horizon = on(FRIRL_HIP_PERTURB_HORIZON) && ex ? const_cast<int32_t *>(ex->horizon) : nullptr;
    a.skip_rules = on(FRIRL_HIP_PERTURB_SKIP_RULES) && hp ? const_cast<int32_t *>(hp->skip_rules) : nullptr;
    a.target = on(FRIRL_HIP_PERTURB_TARGET) && tq ? const_cast<uint8_t *>(tq->target) : nullptr;
    a.expected = on(FRIRL_HIP_PERTURB_EXPECTED) && xp ? const_cast<uint8_t *>(xp->expected) : nullptr;
    a.status = status; a.perturbed = perturbed; a.generation = generation; a.E = E;
    hipStream_t s = as_stream(stream);
    if (perturbed) FRIRL_HIP_TRY(hipMemsetAsync(perturbed, 0, sizeof(int32_t), s), who, return FRIRL_HIP_ELAUNCH);
    if (a.d[0] || a.d[1] || a.d[2] || a.d[3] || a.horizon || a.skip_rules || a.target || a.expected)
        hipLaunchKernelGGL(frirl::perturb_rows_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, a);
    return check_launch(who);
}
