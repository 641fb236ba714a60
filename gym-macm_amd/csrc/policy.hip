// policy.hip — a learned MLP policy over observation rows (macm_policy_flock): the decision of
// policy_mlp.hpp for every row, one lane per row, as bots.hip is for the scripted bot. The first
// actions of a closed loop come from here (on the initial obs), and the per-step loop of the
// workgroup path calls it after every step.
#include "policy_mlp.hpp"

namespace macm {

template <typename OT>
__global__ __launch_bounds__(256) void policy_flock_kernel(PolicyArgs M, const OT* __restrict__ obs, int od,
                                                           long long rows, uint8_t* __restrict__ act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  policy_mlp_row(M, od, obs + i * od, M.noise ? M.noise + i * kPolicyLogits : nullptr, act + i * 3,
                 M.logits ? M.logits + i * kPolicyLogits : nullptr);
}

hipError_t launch_policy_flock(const PolicyArgs& M, const void* obs, bool obs_f64, int od, long long rows,
                               uint8_t* act, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int B = 256;
  const dim3 grid((unsigned)((rows + B - 1) / B));
  if (obs_f64)
    hipLaunchKernelGGL(policy_flock_kernel<double>, grid, dim3(B), 0, s, M, (const double*)obs, od, rows, act);
  else
    hipLaunchKernelGGL(policy_flock_kernel<float>, grid, dim3(B), 0, s, M, (const float*)obs, od, rows, act);
  return hipGetLastError();
}

}  // namespace macm
