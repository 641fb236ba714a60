// Multi-step wave kernels (macm_world_rollout / macm_tdm_rollout): the step body of
// flock_step_w64.hip inside a loop over steps, compiled as its own translation unit with
// -mllvm -disable-machine-licm (see the rollout section of flock_step_w64.hip and the Makefile).
#define MACM_ROLLOUT_TU 1
#define MACM_KS_SWITCH 1  // macm_math.h: the Flock steps of this unit pin their f64 polynomial constants
#include "flock_step_w64.hip"
