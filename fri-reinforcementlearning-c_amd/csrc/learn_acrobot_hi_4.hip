// learn_acrobot_hi_4.hip -- one entry of the persistent learner's launch table (learn_kernel.h: FRIRL_LEARN_SHAPES), a unit of its own for a parallel build.
#include "learn_kernel.h"

FRIRL_LEARN_UNIT(acrobot_hi, 4)
