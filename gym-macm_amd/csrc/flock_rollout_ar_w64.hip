// Multi-step wave kernels of worlds with autoreset on (macm_world_set_autoreset /
// macm_tdm_set_autoreset): the rollout loop of flock_step_w64.hip with the in-launch episode reset
// (rollout_autoreset.inc), in a translation unit of its own so that the kernels of worlds without
// autoreset stay what they are; -mllvm -disable-machine-licm as flock_rollout_w64.hip (Makefile).
#define MACM_ROLLOUT_TU 1
#define MACM_KS_SWITCH 1  // macm_math.h: the Flock steps of this unit pin their f64 polynomial constants
#define MACM_AUTORESET_TU 1
#include "flock_step_w64.hip"
