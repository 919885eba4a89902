// learn_q0.hip -- persistent learner with a per-agent TD target beside the exploration and hyper-parameter rows (learn_kernel.h, ROWS, EXPLORE and TARGET): mountaincar, the twin of learn_i0.hip
#include "learn_kernel.h"

void frirl_learn_launch_mountaincar_target(int H, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                                            const frirl_hip_convergence *cv, const frirl::LearnArgs &la, hipStream_t s)
{
    launch_learn_h<3, 3, FRIRL_HIP_ENV_MOUNTAINCAR, 6, 2, 1, 64, true, true, true>(H, t, b, ag, ev, cv, la, s);
}
