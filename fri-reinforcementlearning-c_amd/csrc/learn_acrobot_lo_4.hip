// learn_acrobot_lo_4.hip -- one entry of the persistent learner's launch table (learn_kernel.h: FRIRL_LEARN_SHAPES), a unit of its own for a parallel build.
#include "learn_kernel.h"

FRIRL_LEARN_UNIT(acrobot_lo, 4)
