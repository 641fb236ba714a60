// policy_sample.hpp — the Gumbel noise a sampling policy draws for itself (include/macm.h,
// macm_sample_config): a counter-based generator, so that the noise of a decision is a function of
// (seed, decision index d, flat row r, head h) alone, however the steps are cut into launches and
// whichever wave runs the env. Shared by the one-shot kernels (policy.hip: macm_policy_noise,
// macm_policy_flock_sampled) and by the sampled rollouts (flock_step_w64.hip / rollout_autoreset.inc):
// one text, inlined everywhere, which is why a sampled launch has the bits of the launch that is
// given macm_policy_noise's output, as ppo_row.hpp is one text for the loss.
//
// The definition:
//   words   w[0..3] = Philox4x32-10(counter = (first_row + r, lo32(d), hi32(d), h), key = (lo32(seed), hi32(seed)));
//           word c < 3 belongs to logit 3h + c, word 3 is unused; r is the flat row of the call or world,
//           first_row the job's row of its row 0 (0 unless the caller names one: the _at entry points), so that
//           a shard of a job draws the job's rows; first_row + rows <= 2^32, the sum never wraps
//   uniform u = ((double)w + 0.5) * 2^-32: exact in float64 and strictly inside (0, 1)
//   noise   g = (float)(-log(-log(u))), both logarithms the device library's float64 log, every
//           operation rounded once (-ffp-contract=off), one final rounding to float32
// Integer arithmetic and plain C++ only; nothing here uses LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace macm {

// The draw of one launch as the kernels take it (a registered macm_sample_config without its padding)
struct SampleArgs {
  unsigned long long seed;
  unsigned long long decision;  // d of the launch's first decision
  uint32_t row0;                // first_row: the job's row of the call's or world's row 0 (a shard's e0 * N)
};

// One row's draw: the key, the decision index and the job's flat row first_row + r, r = e * N + i
struct SampleDraw {
  unsigned long long seed;
  unsigned long long d;
  uint32_t row;
};

// The standard Philox4x32 with 10 rounds (Salmon et al., SC'11): c the counter, k the key, w the output
__device__ __forceinline__ void philox4x32_10(const uint32_t (&c)[4], const uint32_t (&k)[2], uint32_t (&w)[4]) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;  // the round multipliers
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;  // the key's Weyl increments
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)kM0 * c0, p1 = (unsigned long long)kM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kW0;
    k1 += kW1;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

// The four words of head h of a draw
__device__ __forceinline__ void sample_words(const SampleDraw& s, int h, uint32_t (&w)[4]) {
  const uint32_t c[4] = {s.row, (uint32_t)s.d, (uint32_t)(s.d >> 32), (uint32_t)h};
  const uint32_t k[2] = {(uint32_t)s.seed, (uint32_t)(s.seed >> 32)};
  philox4x32_10(c, k, w);
}

// The Gumbel noise of one word
__device__ __forceinline__ float gumbel_of_word(uint32_t w) {
  const double u = ((double)w + 0.5) * 0x1p-32;
  return (float)(-log(-log(u)));
}

// g[c], c < 3: the noise of logits 3h + c of a draw
__device__ __forceinline__ void gumbel_row(const SampleDraw& s, int h, float (&g)[3]) {
  uint32_t w[4];
  sample_words(s, h, w);
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = gumbel_of_word(w[c]);
}

}  // namespace macm
