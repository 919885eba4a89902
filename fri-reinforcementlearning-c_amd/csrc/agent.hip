// agent.hip -- frirl_episode with the caller's environment: frirl_hip_agent_begin / frirl_hip_agent_observe and their taught forms
// (include/frirl_hip.h).
// The kernels are the fused episode kernels of sarsa.hip with EXT = true (episode_kernel.h), instantiated per antecedent count in
// agent_i<N>.hip; agent_call packs their caller's-data argument (ext_io.h) for all of them.
#include "ext_io.h"

using namespace frirl_host;

#define FRIRL_AGENT_NANT_CASES(M) M(2) M(3) M(4) M(5) M(6) M(7) M(8)
#define M(N) void frirl_agent_launch_##N(bool begin, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, \
                                         const frirl_hip_envs *ev, const frirl::ExtIo &io, hipStream_t s);
FRIRL_AGENT_NANT_CASES(M)
#undef M

// everything of an agent call's arguments but the caller's step data and the device (also frirl_hip_learn_demonstration, teach.hip)
int frirl_host::check_agent_shape(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *a, const frirl_hip_envs *ev, const char *who)
{
    if (!t || t->nant < 2 || t->nant > 8) { set_error("%s: nant=%d outside 2..8", who, t ? t->nant : 0); return FRIRL_HIP_EINVAL; }
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!a || !a->grid_values || !a->action_ve) { set_error("%s: NULL agent / grid_values / action_ve", who); return FRIRL_HIP_EINVAL; }
    if (a->A < 1 || a->A > FRIRL_HIP_MAX_ACTIONS) { set_error("%s: A=%d outside 1..%d", who, a->A, FRIRL_HIP_MAX_ACTIONS); return FRIRL_HIP_EINVAL; }
    for (int k = 0; k < t->nant; k++)
        if (a->grid_len[k] < 1 || a->grid_len[k] > FRIRL_HIP_MAX_GRID) { set_error("%s: grid_len[%d]=%d outside 1..%d", who, k, a->grid_len[k], FRIRL_HIP_MAX_GRID); return FRIRL_HIP_EINVAL; }
    if (a->grid_len[t->nant - 1] != a->A) { set_error("%s: the action grid has %d values, A=%d", who, a->grid_len[t->nant - 1], a->A); return FRIRL_HIP_EINVAL; }
    if (!ev || !ev->states || !ev->q_ant || !ev->fus || !ev->done || !ev->ep_steps || !ev->ep_reward) { set_error("%s: NULL env state", who); return FRIRL_HIP_EINVAL; }
    return FRIRL_HIP_OK;
}

static int check_agent_call(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *a, const frirl_hip_envs *ev,
                            const frirl_hip_agent_io *io, bool begin, const char *who)
{
    const int rc = check_agent_shape(t, b, a, ev, who);
    if (rc) return rc;
    if (!io || !io->obs || !io->action_out) { set_error("%s: NULL io / io->obs / io->action_out", who); return FRIRL_HIP_EINVAL; }
    if (!begin && (!io->reward || !io->success)) { set_error("%s: NULL io->reward / io->success", who); return FRIRL_HIP_EINVAL; }
    return check_device();
}

static int agent_call(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_envs *envs,
                      const frirl_hip_agent_io *io, const int32_t *teacher, void *stream, bool begin, const char *who, const frirl_hip_hparam_rows *rows = nullptr,
                      const frirl_hip_explore_rows *explore = nullptr, const frirl_hip_target_rows *target = nullptr,
                      const frirl_hip_expect_rows *expect = nullptr)
{
    int rc = check_agent_call(t, b, agent, envs, io, begin, who);
    if (rc) return rc;
    frirl::ExtIo x;
    static_cast<frirl_hip_agent_io &>(x) = *io;
    x.teacher = teacher;
    x.rows = rows ? *rows : frirl_hip_hparam_rows{};
    x.ex = explore ? *explore : frirl_hip_explore_rows{};
    x.tq = target ? *target : frirl_hip_target_rows{};
    x.xp = expect ? *expect : frirl_hip_expect_rows{};
    switch (t->nant) {
#define M(N) case N: frirl_agent_launch_##N(begin, t, b, agent, envs, x, as_stream(stream)); break;
        FRIRL_AGENT_NANT_CASES(M)
#undef M
    }
    return check_launch(who);
}

extern "C" int frirl_hip_agent_begin(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                     const frirl_hip_envs *envs, const frirl_hip_agent_io *io, void *stream)
{
    return agent_call(t, b, agent, envs, io, nullptr, stream, true, "frirl_hip_agent_begin");
}

extern "C" int frirl_hip_agent_observe(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                       const frirl_hip_envs *envs, const frirl_hip_agent_io *io, void *stream)
{
    return agent_call(t, b, agent, envs, io, nullptr, stream, false, "frirl_hip_agent_observe");
}

// imitation (frirl_episode.c:58-79,127-151): teacher[e] in 0..A-1 replaces row e's epsilon-greedy action; NULL = the untaught call
extern "C" int frirl_hip_agent_begin_taught(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                            const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, true, "frirl_hip_agent_begin_taught");
}

extern "C" int frirl_hip_agent_observe_taught(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                              const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, false, "frirl_hip_agent_observe_taught");
}

// per-agent hyper-parameters (frirl_hip_hparam_rows): row e learns under its own alpha, gamma, insertion bounds, spread threshold and
// skip_rules where a column is given; NULL rows = the taught call
extern "C" int frirl_hip_agent_begin_rows(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                          const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, true, "frirl_hip_agent_begin_rows", rows);
}

extern "C" int frirl_hip_agent_observe_rows(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                            const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, false, "frirl_hip_agent_observe_rows", rows);
}

// per-agent exploration (frirl_hip_explore_rows): row e picks at its own rate, annealed over its own horizon; NULL explore = the _rows call
extern "C" int frirl_hip_agent_begin_explore(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                             const frirl_hip_explore_rows *explore, const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher,
                                             void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, true, "frirl_hip_agent_begin_explore", rows, explore);
}

extern "C" int frirl_hip_agent_observe_explore(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                               const frirl_hip_explore_rows *explore, const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher,
                                               void *stream)
{
    return agent_call(t, b, agent, envs, io, teacher, stream, false, "frirl_hip_agent_observe_explore", rows, explore);
}

// per-agent TD target (frirl_hip_target_rows): row e learns towards Q(s', a') or Q(s', g); NULL target = the _explore call.  No _begin_target:
// begin performs no update
extern "C" int frirl_hip_agent_observe_target(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                              const frirl_hip_explore_rows *explore, const frirl_hip_target_rows *target, const frirl_hip_envs *envs,
                                              const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    if (!target) return frirl_hip_agent_observe_explore(t, b, agent, rows, explore, envs, io, teacher, stream);
    return agent_call(t, b, agent, envs, io, teacher, stream, false, "frirl_hip_agent_observe_target", rows, explore, target);
}

// per-agent expected SARSA (frirl_hip_expect_rows): a flagged row e learns towards the expectation of Q(s', .) under its own pick; NULL
// expect = the _target call.  No _begin_expect: begin performs no update
extern "C" int frirl_hip_agent_observe_expect(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent, const frirl_hip_hparam_rows *rows,
                                              const frirl_hip_explore_rows *explore, const frirl_hip_target_rows *target, const frirl_hip_expect_rows *expect,
                                              const frirl_hip_envs *envs, const frirl_hip_agent_io *io, const int32_t *teacher, void *stream)
{
    if (!expect) return frirl_hip_agent_observe_target(t, b, agent, rows, explore, target, envs, io, teacher, stream);
    return agent_call(t, b, agent, envs, io, teacher, stream, false, "frirl_hip_agent_observe_expect", rows, explore, target, expect);
}
