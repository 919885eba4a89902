// policy_batch_i7.hip -- the caller-stepped per-agent-rule-base step kernels (policy_batch_kernel.h) for 7 antecedents, one file per count for a parallel build.
#include "policy_batch_kernel.h"

void frirl_policy_batch_launch_7(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl::PolicyBatchArgs *pa,
                                 const frirl_hip_agent_io *io, int begin, int nlist, int H, const frirl::PolicyStartsArgs *st, hipStream_t s)
{
    frirl::launch_policy_batch_n<7>(t, b, ag, pa, io, begin, nlist, H, st, s);
}
