// clone.hip -- selection inside a population (include/frirl_hip.h, "select within a population"):
//   frirl_hip_clone_agents  agent e becomes a copy of the learner state of agent src[e], decided and done on the device
//   frirl_hip_select_plan   the src table of a truncation selection from the scores of frirl_hip_batch_evaluate (host only)
//
// The copy is a bandwidth kernel: per cloned agent it moves max(old nrules[e], nrules[src[e]]) columns of every row that belongs to the
// rule base (the (nant + 1) rows of rb, the nant rows of rant and uidx, prev_rconc and weights), columns beyond the source's count as
// zeros, in 16-byte units spread over several workgroups.  Nothing in it depends on the order in which workgroups run: a source is
// never a destination (CHAINED), and the copy kernel writes no per-agent scalar -- every workgroup of a destination reads the same
// old nrules[e] / prev_nrules[e]; clone_finish_kernel, behind it on the stream, writes the scalars.
#include <algorithm>
#include <vector>

#include "device_common.h"

using namespace frirl_host;

namespace frirl {

// what happens to agent e: a function of src and of the sources' rule counts alone, neither of which a clone writes
__device__ __forceinline__ int clone_status(const int32_t *__restrict__ src, const int32_t *__restrict__ nrules, int e, int E, int maxR, int *s_out, int *ns_out)
{
    const int s = src[e];
    *s_out = s;
    *ns_out = 0;
    if (s == e) return FRIRL_HIP_CLONE_KEPT;
    if (s < 0 || s >= E) return FRIRL_HIP_CLONE_BAD_SRC;
    if (src[s] != s) return FRIRL_HIP_CLONE_CHAINED;
    const int ns = nrules[s];
    if (ns < 1 || ns > maxR) return FRIRL_HIP_CLONE_BAD_RULES;
    *ns_out = ns;
    return FRIRL_HIP_CLONE_CLONED;
}

// a destination's own count as a column bound: a count outside 0..maxR says nothing about the row, which is then rewritten whole
__device__ __forceinline__ int clone_bound(int n, int maxR) { return (n < 0 || n > maxR) ? maxR : n; }

// unit u (K elements of T, moved as one V) of a row: dst[c] = c < ns ? src[c] : 0 for the columns c < cols of the unit
template <typename V, typename T, int K>
__device__ __forceinline__ void clone_unit(T *__restrict__ dst, const T *__restrict__ src, int ns, int cols, int u)
{
    const int c0 = u * K;
    if (c0 + K <= ns) {
        *reinterpret_cast<V *>(dst + c0) = __builtin_nontemporal_load(reinterpret_cast<const V *>(src + c0));
    } else if (c0 >= ns && c0 + K <= cols) {
        V z = {};
        *reinterpret_cast<V *>(dst + c0) = z;
    } else {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int c = c0 + j;
            if (c < cols) dst[c] = c < ns ? src[c] : T(0);
        }
    }
}

struct CloneArgs {
    double *rb, *rant, *prev_rconc, *weights;      // rb never NULL; the others NULL = not copied
    uint16_t *uidx;
    const int32_t *nrules, *prev_nrules, *src;
    int32_t E, maxR, nant, G;                       // G workgroups per destination
    int32_t uidx_wide;                              // uidx rows are 16-byte aligned (maxR % 8 == 0 and an aligned base)
};

typedef double clone_d2 __attribute__((ext_vector_type(2)));
typedef uint32_t clone_u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void clone_copy_kernel(const CloneArgs a)
{
    const int e = blockIdx.x / a.G, g = blockIdx.x - e * a.G;
    int s, ns;
    if (clone_status(a.src, a.nrules, e, a.E, a.maxR, &s, &ns) != FRIRL_HIP_CLONE_CLONED) return;
    const size_t M = (size_t)a.maxR;
    const int n = a.nant;
    const int cols = max(clone_bound(a.nrules[e], a.maxR), ns);
    const int cols_prev = a.prev_rconc ? max(cols, clone_bound(a.prev_nrules[e], a.maxR)) : 0;
    // the double rows, in units of two columns: rb (n + 1), rant (n), weights (1) over `cols`, then prev_rconc over `cols_prev`
    const int rows_rb = n + 1, rows_rant = a.rant ? n : 0, rows_w = a.weights ? 1 : 0;
    const int rows = rows_rb + rows_rant + rows_w;
    const int cu = (cols + 1) >> 1, cup = (cols_prev + 1) >> 1;
    // the index mirror, in units of eight columns (16 bytes) or of two (4 bytes: maxR is even, so a row starts on a 4-byte boundary)
    const int ku = a.uidx ? (a.uidx_wide ? (cols + 7) >> 3 : (cols + 1) >> 1) : 0;
    const int n_d = rows * cu, n_p = cup, n_u = n * ku;
    const int total = n_d + n_p + n_u;
    const int stride = a.G * 256;
    for (int i = g * 256 + (int)threadIdx.x; i < total; i += stride) {
        if (i < n_d) {
            const int row = i / cu, u = i - row * cu;
            double *dst;
            const double *sp;
            if (row < rows_rb) {
                dst = a.rb + ((size_t)e * rows_rb + row) * M;
                sp = a.rb + ((size_t)s * rows_rb + row) * M;
            } else if (row < rows_rb + rows_rant) {
                dst = a.rant + ((size_t)e * n + (row - rows_rb)) * M;
                sp = a.rant + ((size_t)s * n + (row - rows_rb)) * M;
            } else {
                dst = a.weights + (size_t)e * M;
                sp = a.weights + (size_t)s * M;
            }
            clone_unit<clone_d2, double, 2>(dst, sp, ns, cols, u);
        } else if (i < n_d + n_p) {
            // the snapshot of the convergence test is retaken from the NEW consequents (teach_reset_kernel, batch.hip)
            clone_unit<clone_d2, double, 2>(a.prev_rconc + (size_t)e * M, a.rb + ((size_t)s * rows_rb + n) * M, ns, cols_prev, i - n_d);
        } else {
            const int j = i - n_d - n_p;
            const int row = j / ku, u = j - row * ku;
            uint16_t *dst = a.uidx + ((size_t)e * n + row) * M;
            const uint16_t *sp = a.uidx + ((size_t)s * n + row) * M;
            if (a.uidx_wide) clone_unit<clone_u4, uint16_t, 8>(dst, sp, ns, cols, u);
            else clone_unit<uint32_t, uint16_t, 2>(dst, sp, ns, cols, u);
        }
    }
}

struct CloneScalars {
    int32_t *nrules, *fus, *spread_R, *status;
    double *spread_ant;
    frirl_hip_convergence conv;                     // conv.prev_nrules == NULL: no convergence state
    const int32_t *src;
    int32_t E, maxR, nant;
};

// behind the copy on the same stream: the per-agent scalars of the cloned agents, and status for everybody
__global__ __launch_bounds__(256) void clone_finish_kernel(const CloneScalars a)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    int s, ns;
    const int st = clone_status(a.src, a.nrules, e, a.E, a.maxR, &s, &ns);
    if (a.status) a.status[e] = st;
    if (st != FRIRL_HIP_CLONE_CLONED) return;
    a.nrules[e] = ns;
    if (a.fus) a.fus[e] = a.fus[s];
    if (a.spread_R) a.spread_R[e] = a.spread_R[s];
    if (a.spread_ant)
        for (int k = 0; k < a.nant; k++) a.spread_ant[(size_t)e * a.nant + k] = a.spread_ant[(size_t)s * a.nant + k];
    if (a.conv.prev_nrules) {
        a.conv.prev_nrules[e] = ns;
        a.conv.prev_steps[e] = -1;
        a.conv.prev_reward[e] = -1.0;
        a.conv.converged[e] = 0;
        if (a.conv.epended) a.conv.epended[e] = 0;
    }
}

}  // namespace frirl

extern "C" int frirl_hip_clone_agents(const frirl_hip_rulebases *b, int32_t nant, const frirl_hip_envs *envs, const frirl_hip_convergence *conv, double *weights,
                                      const int32_t *src, int32_t *status, void *stream)
{
    static const char *who = "frirl_hip_clone_agents";
    if (!b || !b->rb || !b->nrules || !src) { set_error("%s: NULL argument (b, b->rb, b->nrules, src)", who); return FRIRL_HIP_EINVAL; }
    if (nant < 2 || nant > 9) { set_error("%s: nant=%d outside 2..9", who, nant); return FRIRL_HIP_EINVAL; }
    if (b->E < 1) { set_error("%s: E=%d < 1", who, b->E); return FRIRL_HIP_EINVAL; }
    if (b->maxR < 2 || (b->maxR & 1)) { set_error("%s: maxR=%d is odd or below 2 (rows are moved in 16-byte units)", who, b->maxR); return FRIRL_HIP_EINVAL; }
    if (conv && (!conv->prev_nrules || !conv->prev_steps || !conv->prev_reward || !conv->prev_rconc || !conv->converged)) {
        set_error("%s: conv with a NULL array (only epended may be NULL)", who);
        return FRIRL_HIP_EINVAL;
    }
    const void *wide[] = {b->rb, envs ? envs->rant : nullptr, conv ? conv->prev_rconc : nullptr, weights};
    static const char *wide_names[] = {"b->rb", "envs->rant", "conv->prev_rconc", "weights"};
    for (int i = 0; i < 4; i++)
        if (reinterpret_cast<uintptr_t>(wide[i]) & 15) { set_error("%s: %s is not 16-byte aligned", who, wide_names[i]); return FRIRL_HIP_EINVAL; }
    if (reinterpret_cast<uintptr_t>(b->uidx) & 3) { set_error("%s: b->uidx is not 4-byte aligned", who); return FRIRL_HIP_EINVAL; }
    const int rc = check_device();
    if (rc) return rc;
    frirl::CloneArgs a = {};
    a.rb = b->rb; a.rant = envs ? envs->rant : nullptr; a.prev_rconc = conv ? conv->prev_rconc : nullptr; a.weights = weights;
    a.uidx = b->uidx; a.nrules = b->nrules; a.prev_nrules = conv ? conv->prev_nrules : nullptr; a.src = src;
    a.E = b->E; a.maxR = b->maxR; a.nant = nant;
    a.uidx_wide = (b->uidx && b->maxR % 8 == 0 && (reinterpret_cast<uintptr_t>(b->uidx) & 15) == 0) ? 1 : 0;
    // workgroups per destination: enough for about eight per CU when few agents are cloned, never more than the 16-byte units of a
    // full slab give one unit per thread
    const int64_t rows_d = (int64_t)(nant + 1) + (a.rant ? nant : 0) + (weights ? 1 : 0) + (conv ? 1 : 0);
    const int64_t units = rows_d * (b->maxR / 2) + (b->uidx ? (int64_t)nant * ((b->maxR + 7) / 8) : 0);
    const int64_t by_work = std::max<int64_t>(1, (units + 255) / 256), by_chip = std::max<int64_t>(1, (2048 + b->E - 1) / b->E);
    a.G = (int32_t)std::min<int64_t>(std::min(by_work, by_chip), 64);
    if ((int64_t)b->E * a.G > INT32_MAX) { set_error("%s: E=%d is too large", who, b->E); return FRIRL_HIP_EINVAL; }
    frirl::CloneScalars f = {};
    f.nrules = b->nrules; f.fus = envs ? envs->fus : nullptr; f.spread_R = envs ? envs->spread_R : nullptr; f.status = status;
    f.spread_ant = envs ? envs->spread_ant : nullptr;
    if (conv) f.conv = *conv;
    f.src = src; f.E = b->E; f.maxR = b->maxR; f.nant = nant;
    hipLaunchKernelGGL(frirl::clone_copy_kernel, dim3((unsigned)(b->E * a.G)), dim3(256), 0, as_stream(stream), a);
    hipLaunchKernelGGL(frirl::clone_finish_kernel, dim3((unsigned)((b->E + 255) / 256)), dim3(256), 0, as_stream(stream), f);
    return check_launch(who);
}

// rank of the eligible agents by frirl_hip_batch_evaluate's rule, then the worst `replace` take the best `parents` in turn
extern "C" int frirl_hip_select_plan(const frirl_hip_rollout_score *scores, int32_t E, const uint8_t *eligible, int32_t parents, int32_t replace, int32_t *src,
                                     int32_t *rank)
{
    static const char *who = "frirl_hip_select_plan";
    if (!scores || !src) { set_error("%s: NULL scores or src", who); return FRIRL_HIP_EINVAL; }
    if (E < 1) { set_error("%s: E=%d < 1", who, E); return FRIRL_HIP_EINVAL; }
    if (parents < 1) { set_error("%s: parents=%d < 1", who, parents); return FRIRL_HIP_EINVAL; }
    if (replace < 0) { set_error("%s: replace=%d < 0", who, replace); return FRIRL_HIP_EINVAL; }
    std::vector<int32_t> order;
    for (int32_t e = 0; e < E; e++) {
        if (eligible && !eligible[e]) continue;
        if (scores[e].reward_sum != scores[e].reward_sum) { set_error("%s: agent %d: reward_sum is NaN", who, e); return FRIRL_HIP_EINVAL; }
        order.push_back(e);
    }
    const int64_t N = (int64_t)order.size();
    if ((int64_t)parents + replace > N) {
        set_error("%s: parents=%d + replace=%d exceeds the %lld eligible agents (a parent would be replaced)", who, parents, replace, (long long)N);
        return FRIRL_HIP_EINVAL;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {       // stable over ascending indices: the lowest index wins a tie
        if (scores[x].successes != scores[y].successes) return scores[x].successes > scores[y].successes;
        return scores[x].reward_sum > scores[y].reward_sum;
    });
    for (int32_t e = 0; e < E; e++) src[e] = e;
    for (int32_t k = 0; k < replace; k++) src[order[N - 1 - k]] = order[k % parents];
    if (rank) std::copy(order.begin(), order.end(), rank);
    return FRIRL_HIP_OK;
}
