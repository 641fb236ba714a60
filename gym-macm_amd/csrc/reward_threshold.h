// reward_threshold.h — the binary reward's distance test without a square root (host side, C or C++).
//
// The reference gives reward 1 where sqrt((double)td2) < reward_radius, td2 the float32 squared
// distance to the target (mvmnt.py:160-179). A correctly rounded sqrt is monotone, so the set of
// float32 td2 that pass is everything below one float32 threshold
//     T = the smallest float32 with sqrt((double)T) >= R,
// and td2 < T decides the same for every td2: +inf passes neither test when T = +inf, and NaN
// neither at any T. The host computes T once per world (macm_world_create); the wave kernels
// compare (flock_step_w64.hip). tools/reward_thr_check.c prints T for tests/test_reward_threshold.py.
#pragma once
#include <math.h>

static inline float macm_reward_thr2(double R) {
  if (!(R > 0.0)) return 0.0f;  // R <= 0 or NaN: no distance is below it
  if (isinf(R)) return INFINITY;  // every finite distance is
  float T = (float)(R * R);  // within a few ulps of the answer (+inf or 0 beyond float32's range)
  while (sqrt((double)T) < R) T = nextafterf(T, INFINITY);
  while (T > 0.0f && sqrt((double)nextafterf(T, -INFINITY)) >= R) T = nextafterf(T, -INFINITY);
  return T;
}
