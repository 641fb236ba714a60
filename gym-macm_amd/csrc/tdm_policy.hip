// tdm_policy.hip — a learned set policy over TDM observation rows (macm_policy_tdm): the decision of
// tdm_policy.hpp for every agent row, one lane per row, as bots.hip's bots_combat_kernel is for the
// scripted bot. The first actions of a closed loop come from here (on the initial obs), and the
// per-step loop of the workgroup path calls it after every step, over the bot's actions.
#include "tdm_policy.hpp"

namespace macm {

template <typename OT>
__global__ __launch_bounds__(256) void policy_tdm_kernel(TdmPolicyArgs M, const OT* __restrict__ obs,
                                                         const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ health, int N, long long rows,
                                                         const uint8_t* __restrict__ agents,
                                                         const uint8_t* __restrict__ reset, double init_health,
                                                         uint8_t* __restrict__ act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  if (agents && !agents[i % N]) return;  // another actor's row: its action bytes and logits stay
  const double h = reset && reset[i / N] ? init_health : health[i];
  tdm_policy_row<OT, false>(M, obs + i * (N - 1) * 4, mask + i * (N - 1), N, (float)h,
                            M.noise ? M.noise + i * kTdmPolicyLogits : nullptr, act + i * 4,
                            M.logits ? M.logits + i * kTdmPolicyLogits : nullptr);
}

hipError_t launch_policy_tdm(const TdmPolicyArgs& M, const void* obs, const uint8_t* mask, const double* health,
                             bool obs_f64, int N, long long rows, const uint8_t* agents, const uint8_t* reset,
                             double init_health, uint8_t* act, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int B = 256;
  const dim3 grid((unsigned)((rows + B - 1) / B));
  if (obs_f64)
    hipLaunchKernelGGL(policy_tdm_kernel<double>, grid, dim3(B), 0, s, M, (const double*)obs, mask, health, N, rows,
                       agents, reset, init_health, act);
  else
    hipLaunchKernelGGL(policy_tdm_kernel<float>, grid, dim3(B), 0, s, M, (const float*)obs, mask, health, N, rows,
                       agents, reset, init_health, act);
  return hipGetLastError();
}

}  // namespace macm
