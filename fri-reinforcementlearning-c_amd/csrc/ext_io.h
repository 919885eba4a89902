// ext_io.h -- the caller's-data argument of the fused episode kernels (episode_kernel.h), apart from them so that agent.hip can pack it
// without parsing a kernel.
#pragma once

#include <type_traits>

#include "device_common.h"

namespace frirl {

// the caller's step data (frirl_hip_agent_io) for EXT kernels, nothing for the demo kernels
struct NoIo {};
// ... plus the teacher's actions of frirl_hip_agent_begin_taught / _observe_taught: [E] action indices, or NULL (the untaught calls)
// ... and the per-agent hyper-parameters of frirl_hip_agent_begin_rows / _observe_rows: columns [E] or NULL (all NULL: the calls without rows)
// ... and the per-agent exploration of frirl_hip_agent_begin_explore / _observe_explore: columns [E] or NULL (agent->epsilon, horizon_all)
// ... and the per-agent TD target of frirl_hip_agent_observe_target: column [E] or NULL (target_all; all zero: SARSA, the _explore call)
// ... and the per-agent expected-SARSA flags of frirl_hip_agent_observe_expect: column [E] or NULL (expected_all; all zero: the _target call)
struct ExtIo : frirl_hip_agent_io {
    const int32_t *teacher;
    frirl_hip_hparam_rows rows;
    frirl_hip_explore_rows ex;
    frirl_hip_target_rows tq;
    frirl_hip_expect_rows xp;
};
template <bool EXT>
using IoArg = std::conditional_t<EXT, ExtIo, NoIo>;

}  // namespace frirl
