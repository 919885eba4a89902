// learn_q1.hip -- persistent learner with a per-agent TD target beside the exploration and hyper-parameter rows (learn_kernel.h, ROWS, EXPLORE and TARGET): acrobot, 1 .. 8 lanes per agent, the twin of learn_i1.hip
#include "learn_kernel.h"

void frirl_learn_launch_acrobot_lo_target(int H, const frirl_hip_tables *t, const frirl_hip_rulebases *b, const frirl_hip_agent *ag, const frirl_hip_envs *ev,
                                           const frirl_hip_convergence *cv, const frirl::LearnArgs &la, hipStream_t s)
{
    launch_learn_h<5, 3, FRIRL_HIP_ENV_ACROBOT, 6, 2, 1, 8, true, true, true>(H, t, b, ag, ev, cv, la, s);
}
