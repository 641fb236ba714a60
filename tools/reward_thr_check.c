// The host's float32 threshold of the binary reward (gym-macm_amd/csrc/reward_threshold.h), for
// tests/test_reward_threshold.py: reads reward radii as 16-digit hex bit patterns of float64, one
// per line, and prints each one's threshold as an 8-digit hex bit pattern of float32.
//   gcc -O2 -ffp-contract=off -o reward_thr_check tools/reward_thr_check.c -lm
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../gym-macm_amd/csrc/reward_threshold.h"

int main(void) {
  unsigned long long bits;
  while (scanf("%llx", &bits) == 1) {
    uint64_t b = bits;
    double R;
    memcpy(&R, &b, sizeof R);
    const float T = macm_reward_thr2(R);
    uint32_t t;
    memcpy(&t, &T, sizeof t);
    printf("%08x\n", t);
  }
  return 0;
}
