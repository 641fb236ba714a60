// policy.hip — a learned MLP policy over observation rows (macm_policy_flock): the decision of
// policy_mlp.hpp for every row, one lane per row, as bots.hip is for the scripted bot. The first
// actions of a closed loop come from here (on the initial obs), and the per-step loop of the
// workgroup path calls it after every step. Beside it the same decision with the Gumbel draw inside
// (macm_policy_flock_sampled) and the noise of that draw as a tensor (macm_policy_noise), both on
// policy_sample.hpp; the critic over rows (macm_value_flock) and the advantages of a trajectory (macm_gae).
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

// policy_flock_kernel with the draw inside (macm_policy_flock_sampled): row i draws at decision S.decision
template <typename OT>
__global__ __launch_bounds__(256) void policy_flock_sampled_kernel(PolicyArgs M, SampleArgs S, const OT* __restrict__ obs,
                                                                   int od, long long rows, uint8_t* __restrict__ act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  policy_mlp_row<OT, true>(M, od, obs + i * od, nullptr, act + i * 3, M.logits ? M.logits + i * kPolicyLogits : nullptr,
                           SampleDraw{S.seed, S.decision, S.row0 + (uint32_t)i});
}

hipError_t launch_policy_flock_sampled(const PolicyArgs& M, const SampleArgs& S, const void* obs, bool obs_f64, int od,
                                       long long rows, uint8_t* act, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int B = 256;
  const dim3 grid((unsigned)((rows + B - 1) / B));
  if (obs_f64)
    hipLaunchKernelGGL(policy_flock_sampled_kernel<double>, grid, dim3(B), 0, s, M, S, (const double*)obs, od, rows, act);
  else
    hipLaunchKernelGGL(policy_flock_sampled_kernel<float>, grid, dim3(B), 0, s, M, S, (const float*)obs, od, rows, act);
  return hipGetLastError();
}

// The noise itself (macm_policy_noise): thread = row, blockIdx.y strides over the decisions; the words
// as the generator gave them beside it, for the tests
constexpr int kNoiseMaxGridY = 65535;
__global__ __launch_bounds__(256) void policy_noise_kernel(SampleArgs S, long long n_dec, long long rows,
                                                           float* __restrict__ noise, uint32_t* __restrict__ words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  for (long long j = blockIdx.y; j < n_dec; j += gridDim.y) {
    const SampleDraw sd{S.seed, S.decision + (unsigned long long)j, S.row0 + (uint32_t)i};
    const size_t at = (size_t)j * (size_t)rows + (size_t)i;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      float g[3];
      gumbel_row(sd, h, g);
#pragma unroll
      for (int c = 0; c < 3; ++c) noise[at * kPolicyLogits + 3 * h + c] = g[c];
      if (words) {
        uint32_t w[4];
        sample_words(sd, h, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) words[(at * 3 + h) * 4 + q] = w[q];
      }
    }
  }
}

hipError_t launch_policy_noise(const SampleArgs& S, long long n_dec, long long rows, float* noise, uint32_t* words,
                               hipStream_t s) {
  if (n_dec <= 0 || rows <= 0) return hipSuccess;
  const int B = 256;
  const dim3 grid((unsigned)((rows + B - 1) / B), (unsigned)(n_dec < kNoiseMaxGridY ? n_dec : kNoiseMaxGridY));
  hipLaunchKernelGGL(policy_noise_kernel, grid, dim3(B), 0, s, S, n_dec, rows, noise, words);
  return hipGetLastError();
}

// V(obs) of the critic for every row: lane = row, as policy_flock_kernel
template <typename OT>
__global__ __launch_bounds__(256) void value_flock_kernel(ValueArgs V, const OT* __restrict__ obs, int od,
                                                          long long rows, float* __restrict__ values) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  values[i] = value_mlp_row(V, od, obs + i * od);
}

hipError_t launch_value_flock(const ValueArgs& V, const void* obs, bool obs_f64, int od, long long rows, float* values,
                              hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int B = 256;
  const dim3 grid((unsigned)((rows + B - 1) / B));
  if (obs_f64)
    hipLaunchKernelGGL(value_flock_kernel<double>, grid, dim3(B), 0, s, V, (const double*)obs, od, rows, values);
  else
    hipLaunchKernelGGL(value_flock_kernel<float>, grid, dim3(B), 0, s, V, (const float*)obs, od, rows, values);
  return hipGetLastError();
}

// Generalised advantage estimation (include/macm.h, macm_gae): one thread per (env, agent) column
// walks the K rows downwards. The only dependent chain is one fma per row through `carry`, so the
// loads of kGaeRows rows (reward, values, boot: coalesced across the columns; the env's done byte) are
// issued before their chain steps. 13 B read and 8 B written per agent-step; the indices are 64-bit
// (K E N can pass 2^31).
constexpr int kGaeRows = 4;
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ reward, const float* __restrict__ values,
                                                  const float* __restrict__ boot, const uint8_t* __restrict__ done,
                                                  int K, long long E, int N, float gamma, float gl,
                                                  float* __restrict__ adv, float* __restrict__ ret) {
  const long long cols = E * N;
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  const long long e = c / N;
  float carry = 0.0f;
  for (int k = K; k > 0; k -= kGaeRows) {  // rows k - 1 down to k - kGaeRows (those >= 0)
    float r[kGaeRows], v[kGaeRows], b[kGaeRows];
    uint8_t d[kGaeRows];
#pragma unroll
    for (int i = 0; i < kGaeRows; ++i) {
      if (k - 1 - i >= 0) {
        const long long at = (long long)(k - 1 - i) * cols + c;
        r[i] = reward[at];
        v[i] = values[at];
        b[i] = boot[at];
        d[i] = done[(long long)(k - 1 - i) * E + e];
      }
    }
#pragma unroll
    for (int i = 0; i < kGaeRows; ++i) {
      if (k - 1 - i >= 0) {
        const long long at = (long long)(k - 1 - i) * cols + c;
        const float delta = __builtin_fmaf(gamma, b[i], r[i]) - v[i];
        const float a = d[i] ? delta : __builtin_fmaf(gl, carry, delta);
        adv[at] = a;
        ret[at] = a + v[i];
        carry = a;
      }
    }
  }
}

hipError_t launch_gae(const float* reward, const float* values, const float* boot, const uint8_t* done,
                      const GaeShape& g, float* adv, float* ret, hipStream_t s) {
  const long long cols = g.n_envs * g.n_agents;
  if (g.n_steps <= 0 || cols <= 0) return hipSuccess;
  const int B = 256;
  const float gl = g.gamma * g.lambda;  // one float32 multiply
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((cols + B - 1) / B)), dim3(B), 0, s, reward, values, boot, done,
                     g.n_steps, g.n_envs, g.n_agents, g.gamma, gl, adv, ret);
  return hipGetLastError();
}

}  // namespace macm
