// policy_i8.hip -- the caller-stepped shared-rule-base step kernels (policy_kernel.h) for 8 antecedents, one file per count for a parallel build.
#include "policy_kernel.h"

void frirl_policy_launch_8(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_policy_rows *rows,
                           const frirl_hip_agent_io *io, int begin, int G, int H, hipStream_t s)
{
    frirl::launch_policy_n<8>(t, b, ag, rows, io, begin, G, H, s);
}
