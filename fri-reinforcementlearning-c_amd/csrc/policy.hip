// policy.hip -- a trained rule base in the caller's environment: frirl_hip_policy_begin / _observe (one greedy step of Q caller-stepped
// rows on ONE shared rule base) and the resumable rule-base reduction frirl_hip_reducer_* on top of them (include/frirl_hip.h).
// The kernels are policy_kernel.h, instantiated per antecedent count in policy_i<N>.hip; the reduction's host logic is reduce_plan.h,
// shared with frirl_hip_reduce_shared.
#include "reduce_plan.h"
#include "shape_ladder.h"
#include <new>

using namespace frirl_host;

#define M(N) void frirl_policy_launch_##N(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, \
                                          const frirl_hip_policy_rows *rows, const frirl_hip_agent_io *io, int begin, int G, int H, hipStream_t s);
FRIRL_POLICY_NANT_CASES(M)
#undef M

int frirl_host::check_policy_args(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *a, const char *who)
{
    if (!t || t->nant < 2 || t->nant > 8) { set_error("%s: nant=%d outside 2..8", who, t ? t->nant : 0); return FRIRL_HIP_EINVAL; }
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!a || !a->grid_values || !a->action_ve) { set_error("%s: NULL agent / grid_values / action_ve", who); return FRIRL_HIP_EINVAL; }
    if (a->A < 1 || a->A > FRIRL_HIP_MAX_ACTIONS) { set_error("%s: A=%d outside 1..%d", who, a->A, FRIRL_HIP_MAX_ACTIONS); return FRIRL_HIP_EINVAL; }
    if ((rc = check_grid_len(t, a, who))) return rc;
    if (a->grid_len[t->nant - 1] != a->A) { set_error("%s: the action grid has %d values, A=%d", who, a->grid_len[t->nant - 1], a->A); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

int frirl_host::check_policy_io(const frirl_hip_agent_io *io, bool begin, const char *who)
{
    if (!io || !io->obs || !io->action_out) { set_error("%s: NULL io / io->obs / io->action_out", who); return FRIRL_HIP_EINVAL; }
    if (!begin && (!io->reward || !io->success)) { set_error("%s: NULL io->reward / io->success", who); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

// the forms on ONE shared rule base
static int check_policy_one(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *a, const char *who)
{
    const int rc = check_policy_args(t, b, a, who);
    if (rc) return rc;
    if (b->E != 1) { set_error("%s: needs ONE shared rule base (E == 1), got E=%d", who, b->E); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

// Lanes per row and rule slices per conclusion follow the selection rule of frirl_hip_rollout_shared's tiled kernel (lane_group /
// lane_slices, shape_ladder.h), read from the options policy_group / policy_slices.  Kept as they are after measuring every shape on
// the 367-rule acrobot base (profiles/r07_policy_reduce.md, tools/policy_bench.py): at Q = 1023 the rule chosen there, (4, 8), is
// the fastest call (12.4 us against 16.5 / 47 / 103 us for (4, 4) / (4, 1) / (1, 1)); at Q = 65 536 it chooses (4, 1), 93 us, level
// with the best.
static int policy_call(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_policy_rows *rows,
                       const frirl_hip_agent_io *io, void *stream, bool begin, const char *who)
{
    int rc = check_policy_one(t, b, agent, who);
    if (rc) return rc;
    if (!rows || !rows->done || !rows->ep_steps || !rows->success || !rows->ep_reward) { set_error("%s: NULL row state", who); return FRIRL_HIP_EINVAL; }
    if (rows->Q < 1) { set_error("%s: Q=%d < 1", who, rows->Q); return FRIRL_HIP_EINVAL; }
    if ((rows->exclude_mask == nullptr) != (rows->rule_slot == nullptr)) { set_error("%s: exclude_mask and rule_slot go together", who); return FRIRL_HIP_EINVAL; }
    if ((rc = check_policy_io(io, begin, who)) || (rc = check_device())) return rc;
    const int G = lane_group(opts().policy_group, rows->Q, agent->A), H = lane_slices(opts().policy_slices, rows->Q, G);
    switch (t->nant) {
#define M(N) case N: frirl_policy_launch_##N(t, b, agent, rows, io, begin ? 1 : 0, G, H, as_stream(stream)); break;
        FRIRL_POLICY_NANT_CASES(M)
#undef M
    }
    return check_launch(who);
}

extern "C" int frirl_hip_policy_begin(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                      const frirl_hip_policy_rows *rows, const frirl_hip_agent_io *io, void *stream)
{
    return policy_call(t, b, agent, rows, io, stream, true, "frirl_hip_policy_begin");
}

extern "C" int frirl_hip_policy_observe(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                        const frirl_hip_policy_rows *rows, const frirl_hip_agent_io *io, void *stream)
{
    return policy_call(t, b, agent, rows, io, stream, false, "frirl_hip_policy_observe");
}

// ---- the reduction with the caller's environment ----------------------------------------------------------------------------
struct frirl_hip_reducer {
    enum State { IDLE, OPEN, RUNNING };       // between rounds; next_round called; begin called
    frirl_hip_tables t;
    frirl_hip_rulebases b;
    frirl_hip_agent agent;                    // greedy copy (no_random = 1); max_steps capped after the baseline round
    double reward_good_above, reward_tolerance;
    int max_steps;                            // the caller's
    hipStream_t s;
    ReducePlan plan;
    State state = IDLE;
    bool baseline_done = false;
    int Q = 0;                                // rows of the open round
    void *d_slot = nullptr, *d_mask = nullptr, *d_done = nullptr, *d_steps = nullptr, *d_success = nullptr, *d_reward = nullptr;
    std::vector<int32_t> done, steps;
    std::vector<double> reward;

    ~frirl_hip_reducer()
    {
        for (void *p : {d_slot, d_mask, d_done, d_steps, d_success, d_reward}) if (p) (void)hipFree(p);
    }
    frirl_hip_policy_rows rows() const
    {
        frirl_hip_policy_rows r = {};
        r.Q = Q;
        r.done = static_cast<int32_t *>(d_done);
        r.ep_steps = static_cast<int32_t *>(d_steps);
        r.success = static_cast<int32_t *>(d_success);
        r.ep_reward = static_cast<double *>(d_reward);
        if (baseline_done) { r.exclude_mask = static_cast<const uint32_t *>(d_mask); r.rule_slot = static_cast<const uint8_t *>(d_slot); }
        return r;
    }
};

extern "C" frirl_hip_reducer *frirl_hip_reducer_create(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, double *rant,
                                                       int strategy, double reward_tolerance, int depth, void *stream)
{
    const char *who = "frirl_hip_reducer_create";
    if (check_policy_one(t, b, agent, who)) return nullptr;
    if (strategy != 1 && strategy != 2) { set_error("%s: strategy %d (1 = smallest |Q| first, 2 = largest |Q| first)", who, strategy); return nullptr; }
    if (depth == 0) depth = 10;
    if (depth < 1 || depth > frirl::RW_MAX_DEPTH) { set_error("%s: depth %d outside 1..%d", who, depth, frirl::RW_MAX_DEPTH); return nullptr; }
    if (agent->max_steps < 0) { set_error("%s: max_steps=%d < 0", who, agent->max_steps); return nullptr; }
    if (check_device()) return nullptr;
    frirl_hip_reducer *r = new (std::nothrow) frirl_hip_reducer;
    if (!r) { set_error("%s: out of memory", who); return nullptr; }
    r->t = *t; r->b = *b; r->agent = *agent;
    r->agent.no_random = 1;                                           // the replays are greedy (reduction_state == 1)
    r->reward_good_above = agent->reward_good_above;
    r->reward_tolerance = reward_tolerance;
    r->max_steps = agent->max_steps;
    r->s = as_stream(stream);
    if (r->plan.load(who, t, b, rant, strategy, depth, r->s)) { delete r; return nullptr; }
    const size_t n = (size_t)r->plan.lanes_max();
    if (hipMalloc(&r->d_slot, (size_t)b->maxR) != hipSuccess || hipMalloc(&r->d_mask, sizeof(uint32_t) * n) != hipSuccess ||
        hipMalloc(&r->d_done, sizeof(int32_t) * n) != hipSuccess || hipMalloc(&r->d_steps, sizeof(int32_t) * n) != hipSuccess ||
        hipMalloc(&r->d_success, sizeof(int32_t) * n) != hipSuccess || hipMalloc(&r->d_reward, sizeof(double) * n) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc failed", who);
        delete r;
        return nullptr;
    }
    r->done.resize(n); r->steps.resize(n); r->reward.resize(n);
    return r;
}

extern "C" void frirl_hip_reducer_destroy(frirl_hip_reducer *r) { delete r; }

extern "C" int frirl_hip_reducer_next_round(frirl_hip_reducer *r, int32_t *Q)
{
    const char *who = "frirl_hip_reducer_next_round";
    if (!r || !Q) { set_error("%s: NULL argument", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_reducer::IDLE) { set_error("%s: the previous round has not been closed (frirl_hip_reducer_end_round)", who); return FRIRL_HIP_EINVAL; }
    int lanes = 1;                                                    // round 0: the baseline replay on the un-reduced rule base
    if (r->baseline_done) {
        const int rc = r->plan.open_round(r->d_slot, r->d_mask, r->s, &lanes);
        if (rc) return rc;
    }
    *Q = r->Q = lanes;
    if (lanes > 0) r->state = frirl_hip_reducer::OPEN;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reducer_begin(frirl_hip_reducer *r, const frirl_hip_agent_io *io)
{
    const char *who = "frirl_hip_reducer_begin";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_reducer::OPEN) { set_error("%s: no open round (frirl_hip_reducer_next_round first; one begin per round)", who); return FRIRL_HIP_EINVAL; }
    int rc = check_policy_io(io, true, who);
    if (rc) return rc;
    frirl_hip_agent_io all = *io;
    all.reset = nullptr;                                              // every row of the round starts
    const frirl_hip_policy_rows rows = r->rows();
    if ((rc = frirl_hip_policy_begin(&r->t, &r->b, &r->agent, &rows, &all, r->s))) return rc;
    r->state = frirl_hip_reducer::RUNNING;
    return FRIRL_HIP_OK;
}

// row state of the running round to the host; synchronises.  Returns the rows whose replay has not ended, < 0 on error.
static int reducer_fetch(frirl_hip_reducer *r, const char *who)
{
    const size_t n = (size_t)r->Q;
    if (hipMemcpyAsync(r->done.data(), r->d_done, sizeof(int32_t) * n, hipMemcpyDeviceToHost, r->s) != hipSuccess ||
        hipMemcpyAsync(r->steps.data(), r->d_steps, sizeof(int32_t) * n, hipMemcpyDeviceToHost, r->s) != hipSuccess ||
        hipMemcpyAsync(r->reward.data(), r->d_reward, sizeof(double) * n, hipMemcpyDeviceToHost, r->s) != hipSuccess ||
        hipStreamSynchronize(r->s) != hipSuccess) {
        set_error("%s: reading the row state failed: %s", who, hipGetErrorString(hipGetLastError()));
        return FRIRL_HIP_ELAUNCH;
    }
    int live = 0;
    for (size_t i = 0; i < n; i++) live += r->done[i] == 0;
    return live;
}

extern "C" int frirl_hip_reducer_observe(frirl_hip_reducer *r, const frirl_hip_agent_io *io, int32_t *rows_live)
{
    const char *who = "frirl_hip_reducer_observe";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_reducer::RUNNING) { set_error("%s: no running round (frirl_hip_reducer_begin first)", who); return FRIRL_HIP_EINVAL; }
    const frirl_hip_policy_rows rows = r->rows();
    const int rc = frirl_hip_policy_observe(&r->t, &r->b, &r->agent, &rows, io, r->s);
    if (rc || !rows_live) return rc;
    const int live = reducer_fetch(r, who);
    if (live < 0) return live;
    *rows_live = live;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reducer_end_round(frirl_hip_reducer *r)
{
    const char *who = "frirl_hip_reducer_end_round";
    if (!r) { set_error("%s: NULL reducer", who); return FRIRL_HIP_EINVAL; }
    if (r->state != frirl_hip_reducer::RUNNING) { set_error("%s: no running round", who); return FRIRL_HIP_EINVAL; }
    const int live = reducer_fetch(r, who);
    if (live < 0) return live;
    if (live > 0) { set_error("%s: %d of %d replays have not ended", who, live, r->Q); return FRIRL_HIP_EINVAL; }
    if (!r->baseline_done) {
        r->plan.set_baseline(r->steps[0], r->reward[0]);
        r->agent.max_steps = r->plan.capped_steps(r->max_steps);
        r->baseline_done = true;
    } else {
        const int rc = r->plan.close_round(r->steps.data(), r->reward.data(), r->reward_good_above, r->reward_tolerance, r->s);
        if (rc) return rc;
    }
    r->state = frirl_hip_reducer::IDLE;
    return FRIRL_HIP_OK;
}

extern "C" int frirl_hip_reducer_result(const frirl_hip_reducer *r, int32_t *kept, frirl_hip_reduce_result *result)
{
    if (!r || !result) { set_error("frirl_hip_reducer_result: NULL argument"); return FRIRL_HIP_EINVAL; }
    r->plan.result(kept, result);
    return FRIRL_HIP_OK;
}
