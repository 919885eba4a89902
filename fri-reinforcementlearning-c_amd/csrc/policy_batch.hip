// policy_batch.hip -- EVERY agent's own rule base in the caller's environment: frirl_hip_policy_batch_begin / _observe (one greedy step
// of E * n caller-stepped rows, row q on the rule base of agent q / n) and the resumable batched reduction frirl_hip_batch_reducer_* on
// top of them (include/frirl_hip.h).  The step kernels are policy_batch_kernel.h, instantiated per antecedent count in
// policy_batch_i<N>.hip; the round protocol of the reduction (checks, workspace, order, open, close and result kernels, with or
// without a set of start states) is ReduceRun's (reduce_run.h), the one frirl_hip_reduce_batch and _starts run.  The reducer owns what
// is its own: the IDLE / OPEN / RUNNING state machine, the row flags, and the n = 1 view of _result_starts.  A round is: the caller's
// begin / observe loop, every step ONE launch over the rows of the agents still reducing, then ReduceRun::close (tree walk +
// compaction, the next round's open kernel).  The host reads the 16-byte header only: live agents of the next round, rows still live.
#include "policy_batch_kernel.h"
#include "reduce_run.h"
#include <new>

#define M(N) void frirl_policy_batch_launch_##N(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, \
                                                const frirl::PolicyBatchArgs *pa, const frirl_hip_agent_io *io, int begin, int nlist, int H,     \
                                                const frirl::PolicyStartsArgs *st, hipStream_t s);
FRIRL_POLICY_NANT_CASES(M)
#undef M

// Rule slices per conclusion.  The lanes per row are fixed by the action count (rb_group: 4 for up to 4 actions, else 8; the option
// "policy_group" can name no other); "policy_slices" = 1 / 4 / 8 forces H.  Otherwise one row per agent (the baseline replay) takes a
// full wave per row, and trees take the rule of frirl_hip_reduce_batch (rb_slices: 8 while every row stays resident, else 4, else 1).
static int policy_batch_slices(long rows, int n, int A)
{
    { const int v = opts().policy_slices; if (v == 1 || v == 4 || v == 8) return v; }
    if (n == 1) return FRIRL_WAVE / rb_group(A);
    return rb_slices(rows, A);
}

static void policy_batch_launch(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl::PolicyBatchArgs *pa,
                                const frirl_hip_agent_io *io, int begin, int nlist, hipStream_t s, const frirl::PolicyStartsArgs *st = nullptr)
{
    const int H = policy_batch_slices((long)nlist * pa->rows.n, pa->rows.n, agent->A);
    switch (t->nant) {
#define M(N) case N: frirl_policy_batch_launch_##N(t, b, agent, pa, io, begin, nlist, H, st, s); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
}

static int policy_batch_call(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_policy_batch_rows *rows,
                             const frirl_hip_agent_io *io, void *stream, bool begin, const char *who)
{
    int rc = check_policy_args(t, b, agent, who);
    if (rc) return rc;
    if (!rows || !rows->done || !rows->ep_steps || !rows->success || !rows->ep_reward) { set_error("%s: NULL row state", who); return FRIRL_HIP_EINVAL; }
    if (rows->n < 1 || (long)rows->n * b->E > 0x7fffffffL) { set_error("%s: n=%d < 1 or E * n beyond 2^31 - 1", who, rows->n); return FRIRL_HIP_EINVAL; }
    if ((rows->exclude_mask == nullptr) != (rows->rule_slot == nullptr)) { set_error("%s: exclude_mask and rule_slot go together", who); return FRIRL_HIP_EINVAL; }
    if (rows->agents && (rows->nagents < 1 || rows->nagents > b->E)) { set_error("%s: nagents=%d outside 1..E=%d", who, rows->nagents, b->E); return FRIRL_HIP_EINVAL; }
    if ((rc = check_policy_io(io, begin, who)) || (rc = check_device())) return rc;
    frirl::PolicyBatchArgs pa = {};
    pa.rows = *rows;
    pa.list = rows->agents;
    pa.E = b->E;
    pa.state_stride = rows->n;
    policy_batch_launch(t, b, agent, &pa, io, begin ? 1 : 0, rows->agents ? rows->nagents : b->E, as_stream(stream));
    return check_launch(who);
}

extern "C" int frirl_hip_policy_batch_begin(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                            const frirl_hip_policy_batch_rows *rows, const frirl_hip_agent_io *io, void *stream)
{
    return policy_batch_call(t, b, agent, rows, io, stream, true, "frirl_hip_policy_batch_begin");
}

extern "C" int frirl_hip_policy_batch_observe(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                              const frirl_hip_policy_batch_rows *rows, const frirl_hip_agent_io *io, void *stream)
{
    return policy_batch_call(t, b, agent, rows, io, stream, false, "frirl_hip_policy_batch_observe");
}

// ---- the batched reduction with the caller's environment -------------------------------------------------------------------
namespace frirl {
__global__ void policy_batch_fill_kernel(int32_t *__restrict__ x, int n, int32_t v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

// the n = 1 view of a reducer made without start states: what frirl_hip_batch_reducer_result_starts reports for it.  An agent whose
// baseline replay ran has rollouts > 0; `base` = prev_reward of every agent after round 0.
__global__ void policy_batch_one_start_kernel(int E, ReduceBatchWs ws, const double *__restrict__ base, frirl_hip_reduce_start_result *__restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool ran = ws.rollouts[e] > 0;
    frirl_hip_reduce_start_result r;
    r.used = ran ? 1 : 0;
    r.steps_incremental = ran ? ws.steps_inc[e] : -1;
    r.baseline_reward = ran ? base[e] : 0.0;
    r.reward = ran ? ws.prev[e] : 0.0;
    out[e] = r;
}
}  // namespace frirl

struct frirl_hip_batch_reducer {
    enum State { IDLE, OPEN, RUNNING };       // between rounds; next_round called; begin called
    ReduceRun run;                            // checks, workspace view, header, round number and every protocol kernel
    void *d_ws = nullptr, *d_done = nullptr, *d_success = nullptr, *d_base = nullptr, *d_view = nullptr;
    State state = IDLE;
    int n = 0, Q = 0;                         // rows per agent (with start states: rows of a node x ns) and rows of the open round
    bool live_known = false;                  // run.hdr[3] holds the rows still live after the last launch

    ~frirl_hip_batch_reducer()
    {
        for (void *p : {d_ws, d_done, d_success, d_base, d_view}) if (p) (void)hipFree(p);
    }
    bool starts_round() const { return run.ns && !run.first(); }     // the rows are nodes x starts: PolicyStartsArgs
    frirl::PolicyBatchArgs args() const
    {
        const ReduceBatchWs &ws = run.ws;
        frirl::PolicyBatchArgs pa = {};
        pa.rows.n = n;
        pa.rows.done = static_cast<int32_t *>(d_done);
        pa.rows.success = static_cast<int32_t *>(d_success);
        pa.rows.ep_steps = ws.steps;          // the arrays the close kernel reads: a round ends without a copy
        pa.rows.ep_reward = ws.reward;
        pa.rows.step_cap = ws.cap;
        pa.rows.rows_live = ws.hdr + 3;
        if (run.ns && run.first()) pa.rows.row_count = run.sw.cnt;    // the baseline replays: row k = participating start k
        if (!run.first()) {
            pa.rows.exclude_mask = ws.mask;
            pa.rows.rule_slot = ws.slot;
            pa.depth_of = ws.d;
            pa.mask_by_node = 1;
        }
        pa.list = ws.live[run.cur()];
        pa.E = run.b.E;
        pa.state_stride = ws.nodes * run.per_node();
        return pa;
    }
    frirl::PolicyStartsArgs starts_args() const
    {
        frirl::PolicyStartsArgs st = {};
        st.res = run.sw.res;
        st.cap = run.sw.cap;
        st.ns = run.ns;
        return st;
    }
};

// frirl_hip_batch_reducer_create (starts == NULL) and _create_starts
static frirl_hip_batch_reducer *batch_reducer_create(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                                     const uint8_t *active, const frirl_hip_reduce_starts *starts, int strategy, double reward_tolerance,
                                                     int depth, void *stream, const char *who)
{
    if (check_policy_args(t, b, agent, who)) return nullptr;
    frirl_hip_batch_reducer *r = new (std::nothrow) frirl_hip_batch_reducer;
    if (!r) { set_error("%s: out of memory", who); return nullptr; }
    ReduceRun &run = r->run;
    if (run.init(who, t, b, agent, rant, starts, strategy, reward_tolerance, depth, true, stream) || check_device()) { delete r; return nullptr; }
    const size_t E = (size_t)b->E, rows = E * run.per_node() * run.nodes;
    bool ok = hipMalloc(&r->d_ws, run.need) == hipSuccess && hipMalloc(&r->d_done, sizeof(int32_t) * rows) == hipSuccess &&
              hipMalloc(&r->d_success, sizeof(int32_t) * rows) == hipSuccess;
    if (ok && !starts)                                               // for the n = 1 view of _result_starts
        ok = hipMalloc(&r->d_base, sizeof(double) * E) == hipSuccess && hipMalloc(&r->d_view, sizeof(frirl_hip_reduce_start_result) * E) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc failed", who);
    }
    if (!ok || run.start(who, r->d_ws, active, starts ? starts->start_count : nullptr)) { delete r; return nullptr; }
    return r;
}

extern "C" frirl_hip_batch_reducer *frirl_hip_batch_reducer_create(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                                                   double *rant, const uint8_t *active, int strategy, double reward_tolerance, int depth,
                                                                   void *stream)
{
    return batch_reducer_create(t, b, agent, rant, active, nullptr, strategy, reward_tolerance, depth, stream, "frirl_hip_batch_reducer_create");
}

extern "C" frirl_hip_batch_reducer *frirl_hip_batch_reducer_create_starts(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                                                          double *rant, const uint8_t *active, const frirl_hip_reduce_starts *starts,
                                                                          int strategy, double reward_tolerance, int depth, void *stream)
{
    const char *who = "frirl_hip_batch_reducer_create_starts";
    if (!starts) { set_error("%s: NULL starts", who); return nullptr; }
    return batch_reducer_create(t, b, agent, rant, active, starts, strategy, reward_tolerance, depth, stream, who);
}

extern "C" int frirl_hip_batch_reducer_starts(const frirl_hip_batch_reducer *r) { return r ? r->run.per_node() : 0; }

extern "C" void frirl_hip_batch_reducer_destroy(frirl_hip_batch_reducer *r) { delete r; }

extern "C" int frirl_hip_batch_reducer_next_round(frirl_hip_batch_reducer *r, int32_t *Q, int32_t *rows_per_agent, int32_t *agents_live)
{
    const char *who = "frirl_hip_batch_reducer_next_round";
    if (!r || !Q) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::IDLE) { set_error("%s: the previous round has not been closed (frirl_hip_batch_reducer_end_round)", who); return FRIRL_HIP_EINVAL; }
    const int nlive = r->run.nlive();
    const int n = nlive == 0 ? 0 : r->run.rows_per_agent();
    if (nlive > 0) {                                                  // rows of agents that sit out, and nodes that do not exist, stay done
        const int q = r->run.b.E * n;
        hipLaunchKernelGGL(frirl::policy_batch_fill_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, r->run.s, static_cast<int32_t *>(r->d_done), q, 1);
        const int rc = check_launch(who);
        if (rc) return rc;
        r->state = frirl_hip_batch_reducer::OPEN;
    }
    r->n = n;
    *Q = r->Q = r->run.b.E * n;
    if (rows_per_agent) *rows_per_agent = n;
    if (agents_live) *agents_live = nlive;
    return FRIRL_HIP_OK;
}

static int batch_reducer_step(frirl_hip_batch_reducer *r, const frirl_hip_agent_io *io, int begin, const char *who)
{
    const ReduceRun &run = r->run;
    FRIRL_HIP_TRY(hipMemsetAsync(run.ws.hdr + 3, 0, sizeof(int32_t), run.s), who, return FRIRL_HIP_ELAUNCH);
    const frirl::PolicyBatchArgs pa = r->args();
    const frirl::PolicyStartsArgs st = r->starts_args();
    policy_batch_launch(&run.t, &run.b, &run.agent, &pa, io, begin, run.nlive(), run.s, r->starts_round() ? &st : nullptr);
    r->live_known = false;
    return check_launch(who);
}

extern "C" int frirl_hip_batch_reducer_begin(frirl_hip_batch_reducer *r, const frirl_hip_agent_io *io)
{
    const char *who = "frirl_hip_batch_reducer_begin";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::OPEN) { set_error("%s: no open round (frirl_hip_batch_reducer_next_round first; one begin per round)", who); return FRIRL_HIP_EINVAL; }
    int rc = check_policy_io(io, true, who);
    if (rc) return rc;
    frirl_hip_agent_io all = *io;
    all.reset = nullptr;                                              // every row of the round starts
    if ((rc = batch_reducer_step(r, &all, 1, who))) return rc;
    r->state = frirl_hip_batch_reducer::RUNNING;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reducer_observe(frirl_hip_batch_reducer *r, const frirl_hip_agent_io *io, int32_t *rows_live)
{
    const char *who = "frirl_hip_batch_reducer_observe";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::RUNNING) { set_error("%s: no running round (frirl_hip_batch_reducer_begin first)", who); return FRIRL_HIP_EINVAL; }
    int rc = check_policy_io(io, false, who);
    if (rc || (rc = batch_reducer_step(r, io, 0, who)) || !rows_live) return rc;
    if ((rc = r->run.header(who))) return rc;
    r->live_known = true;
    *rows_live = r->run.hdr[3];
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reducer_end_round(frirl_hip_batch_reducer *r)
{
    const char *who = "frirl_hip_batch_reducer_end_round";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::RUNNING) { set_error("%s: no running round", who); return FRIRL_HIP_EINVAL; }
    ReduceRun &run = r->run;
    int rc;
    if (!r->live_known) {
        if ((rc = run.header(who))) return rc;
        r->live_known = true;
    }
    if (run.hdr[3] > 0) { set_error("%s: %d of %d replays have not ended", who, run.hdr[3], r->Q); return FRIRL_HIP_EINVAL; }
    const bool base = run.first() && !run.ns;                         // keep the baseline rewards for the n = 1 view of _result_starts:
    if ((rc = run.close(who))) return rc;                             // ws.prev holds them until the next round's close kernel
    r->state = frirl_hip_batch_reducer::IDLE;
    if (base) FRIRL_HIP_TRY(hipMemcpyAsync(r->d_base, run.ws.prev, sizeof(double) * run.b.E, hipMemcpyDeviceToDevice, run.s), who, return FRIRL_HIP_ELAUNCH);
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_batch_reducer_result(frirl_hip_batch_reducer *r, int32_t *kept, frirl_hip_reduce_result *results)
{
    const char *who = "frirl_hip_batch_reducer_result";
    if (!r || !results) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::IDLE) { set_error("%s: a round is open (frirl_hip_batch_reducer_end_round first)", who); return FRIRL_HIP_EINVAL; }
    return r->run.results(who, kept, results, nullptr);
}

extern "C" int frirl_hip_batch_reducer_result_starts(frirl_hip_batch_reducer *r, frirl_hip_reduce_start_result *per_start)
{
    const char *who = "frirl_hip_batch_reducer_result_starts";
    if (!r || !per_start) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_batch_reducer::IDLE) { set_error("%s: a round is open (frirl_hip_batch_reducer_end_round first)", who); return FRIRL_HIP_EINVAL; }
    ReduceRun &run = r->run;
    if (run.ns) return run.results(who, nullptr, nullptr, per_start);
    // no per-start arrays: the n = 1 view is built from the per-agent ones
    const int E = run.b.E;
    frirl_hip_reduce_start_result *d_res = static_cast<frirl_hip_reduce_start_result *>(r->d_view);
    hipLaunchKernelGGL(frirl::policy_batch_one_start_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, run.s, E, run.ws, static_cast<const double *>(r->d_base), d_res);
    FRIRL_HIP_TRY(hipMemcpyAsync(per_start, d_res, sizeof(frirl_hip_reduce_start_result) * E, hipMemcpyDeviceToHost, run.s), who, return FRIRL_HIP_ELAUNCH);
    FRIRL_HIP_TRY(hipStreamSynchronize(run.s), who, return FRIRL_HIP_ELAUNCH);
    return check_launch(who);
}

extern "C" const int32_t *frirl_hip_batch_reducer_row_done(const frirl_hip_batch_reducer *r)
{
    return r ? static_cast<const int32_t *>(r->d_done) : nullptr;
}
