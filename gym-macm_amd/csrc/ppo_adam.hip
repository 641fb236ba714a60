// ppo_adam.hip — the optimiser step of the PPO update (include/macm.h, macm_ppo_adam): Adam over both nets'
// params with the global-norm clip, the KL gate and the non-finite guard, in one launch of one workgroup.
//
// Why one workgroup: both nets together have at most 2 x 1,577 params, eleven or twelve elements per thread
// of 256, and the norm of all of them stands before the first element's update. A second workgroup would buy
// a cross-workgroup finish for a few microseconds of arithmetic; what this launch replaces is some twenty
// tiny launches and their host time, not bandwidth.
//
// Arithmetic as ppo_row.hpp's: float64 on the float32 inputs, every operation rounded once
// (-ffp-contract=off, hipflags.mk), in the association written in the header, with + - * / sqrt only, so
// that a numpy float64 restatement (tests/adam_ref.py) has its bits. The powers of the betas are running
// products kept in the state: a pow would be the one operation the reference could not follow exactly.
#include <math.h>

#include "ppo_row.hpp"

namespace macm {

__global__ __launch_bounds__(kAdamBlock) void ppo_adam_kernel(const AdamArgs A) {
  __shared__ double s[kAdamBlock];
  const int tid = threadIdx.x;
  // every read of head stands before the first barrier; thread 0 alone writes it, behind the last
  const double t = A.head[0], h1 = A.head[1], h2 = A.head[2], stopped = A.head[3], skipped = A.head[6];
  if (stopped != 0.0) return;  // (block-uniform, as every return here)
  if (A.stats && A.target_kl > 0.0 && !(A.stats[4] <= A.target_kl)) {
    // the others read head[3] as 0 or as 1: they return here or above
    if (tid == 0) A.head[3] = 1.0;
    return;
  }
  const int n0 = A.n[0], n = n0 + A.n[1];
  double acc = 0.0;
  for (int j = tid; j < n; j += kAdamBlock) {
    const double g = (double)(j < n0 ? A.grad[0][j] : A.grad[1][j - n0]);
    acc = acc + g * g;
  }
  s[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int d = kAdamBlock / 2; d >= 1; d >>= 1) {
    if (tid < d) s[tid] = s[tid] + s[tid + d];
    __syncthreads();
  }
  const double norm = sqrt(s[0]);
  if (!(fabs(norm) <= 1.7976931348623157e308)) {  // inf or NaN
    if (tid == 0) {
      A.head[6] = skipped + 1.0;
      A.head[4] = norm;
    }
    return;
  }
  double coef = 1.0;
  if (A.max_grad_norm > 0.0) {
    const double c = A.max_grad_norm / (norm + 1e-6);
    coef = c < 1.0 ? c : 1.0;
  }
  const double p1 = (t == 0.0 ? 1.0 : h1) * A.beta1, p2 = (t == 0.0 ? 1.0 : h2) * A.beta2;
  const double c1 = 1.0 - p1, c2 = 1.0 - p2;
  for (int j = tid; j < n; j += kAdamBlock) {
    const bool crit = j >= n0;  // (the pointers are selected, not indexed: the argument struct stays in registers)
    const int i = crit ? j - n0 : j;
    const float* const gr = crit ? A.grad[1] : A.grad[0];
    float* const pm = crit ? A.m[1] : A.m[0];
    float* const pv = crit ? A.v[1] : A.v[0];
    float* const pp = crit ? A.param[1] : A.param[0];
    const double g = (double)gr[i] * coef;
    const float m = (float)(A.beta1 * (double)pm[i] + A.omb1 * g);
    const float v = (float)(A.beta2 * (double)pv[i] + A.omb2 * (g * g));
    pm[i] = m;
    pv[i] = v;
    pp[i] = (float)((double)pp[i] - A.lr * (((double)m / c1) / (sqrt((double)v / c2) + A.eps)));
  }
  if (tid == 0) {
    A.head[0] = t + 1.0;
    A.head[1] = p1;
    A.head[2] = p2;
    A.head[4] = norm;
    A.head[5] = coef;
  }
}

hipError_t launch_ppo_adam(const AdamArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(ppo_adam_kernel, dim3(1), dim3(kAdamBlock), 0, s, A);
  return hipGetLastError();
}

}  // namespace macm
