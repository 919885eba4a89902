// teach_i5.hip -- the demonstration replay kernels (teach_kernel.h) for 5 antecedents, one file per count for a parallel build.
#include "teach_kernel.h"

void frirl_teach_launch_5(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                          const frirl_hip_demonstration *dm, int passes, int32_t *replayed, uint8_t *refused, hipStream_t s)
{
    frirl::launch_teach<5>(t, b, ag, ev, dm, passes, replayed, refused, s);
}
