// agent_i6.hip -- the caller's-environment episode kernels (episode_kernel.h, EXT = true) for 6 antecedents, one file per count for a parallel build.
#include "episode_kernel.h"

void frirl_agent_launch_6(bool begin, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                          const frirl::ExtIo &io, hipStream_t s)
{
    if (begin) frirl::launch_episode<6, true, true>(t, b, ag, ev, s, io);
    else frirl::launch_episode<6, false, true>(t, b, ag, ev, s, io);
}
