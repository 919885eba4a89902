// agent_i6.hip -- the caller's-environment episode kernels (episode_kernel.h, EXT = true) for 6 antecedents, one file per count for a parallel build.
#include "episode_kernel.h"

void frirl_agent_launch_6(bool begin, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                          const frirl_hip_agent_io &io, const int32_t *teacher, const frirl_hip_hparam_rows *rows,
                          const frirl_hip_explore_rows *explore, const frirl_hip_target_rows *target, hipStream_t s)
{
    frirl::ExtIo x;
    static_cast<frirl_hip_agent_io &>(x) = io;
    x.teacher = teacher;
    x.rows = rows ? *rows : frirl_hip_hparam_rows{};
    x.ex = explore ? *explore : frirl_hip_explore_rows{};
    x.tq = target ? *target : frirl_hip_target_rows{};
    if (begin) frirl::launch_episode<6, true, true>(t, b, ag, ev, s, x);
    else frirl::launch_episode<6, false, true>(t, b, ag, ev, s, x);
}
