// teach.hip -- frirl_hip_learn_demonstration (include/frirl_hip.h): every agent learns a recorded log of observations, actions and
// rewards in one launch.  The kernel is teach_kernel.h, instantiated per antecedent count in teach_i<N>.hip.
#include "device_common.h"

using namespace frirl_host;

#define FRIRL_TEACH_NANT_CASES(M) M(2) M(3) M(4) M(5) M(6) M(7) M(8)
#define M(N) void frirl_teach_launch_##N(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev, \
                                         const frirl_hip_demonstration *dm, int passes, int32_t *replayed, uint8_t *refused, hipStream_t s);
FRIRL_TEACH_NANT_CASES(M)
#undef M

extern "C" int frirl_hip_learn_demonstration(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *agent,
                                             const frirl_hip_envs *envs, const frirl_hip_demonstration *demo, int32_t passes,
                                             int32_t *replayed, uint8_t *refused, void *stream)
{
    const char *who = "frirl_hip_learn_demonstration";
    if (!demo || !demo->obs || !demo->action || !demo->reward || !demo->success) {
        set_error("%s: NULL demo / obs / action / reward / success", who);
        return FRIRL_HIP_EINVAL;
    }
    if (demo->T < 1) { set_error("%s: T=%d < 1", who, demo->T); return FRIRL_HIP_EINVAL; }
    if (passes < 1 || passes > 1024) { set_error("%s: passes=%d outside 1..1024", who, passes); return FRIRL_HIP_EINVAL; }
    if (demo->agent_stride < 0 || (demo->agent_stride > 0 && demo->agent_stride < demo->T)) {
        set_error("%s: agent_stride=%lld must be 0 (one shared log) or >= T=%d", who, (long long)demo->agent_stride, demo->T);
        return FRIRL_HIP_EINVAL;
    }
    int rc = check_agent_shape(t, b, agent, envs, who);
    if (rc) return rc;
    rc = check_device();
    if (rc) return rc;
    switch (t->nant) {
#define M(N) case N: frirl_teach_launch_##N(t, b, agent, envs, demo, passes, replayed, refused, as_stream(stream)); break;
        FRIRL_TEACH_NANT_CASES(M)
#undef M
    }
    return check_launch(who);
}
