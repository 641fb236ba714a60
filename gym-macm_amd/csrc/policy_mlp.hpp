// policy_mlp.hpp — one agent's decision of a learned policy: a float32 MLP over the agent's obs row,
// shared by the one-shot kernel (policy.hip, macm_policy_flock) and the closed-loop rollouts
// (flock_step_w64.hip / rollout_autoreset.inc, macm_world_rollout_policy), where it stands in the
// place of the scripted bot (bots.hpp); and the critic beside it (macm_value_mlp, below).
//
// The definition (include/macm.h, macm_policy_mlp), all float32:
//   x[q]  = (float)obs[q], q < OD (a float64 obs rounds to nearest)
//   layer : acc = b[j]; acc = fmaf(W[k][j], x[k], acc) for k ascending; one rounding per step
//   hidden: relu(v) = v > 0 ? v : +0.0f (so -0 and NaN give +0); the output layer has none
//   head h: z[c] = logits[3h + c] (+ noise[3h + c]); action[h] = the lowest c with the largest z,
//           by `z[c] > best` from best = -inf, so a NaN is never chosen over a number
// lane = row: every weight is a wave-uniform operand. The params are read through the constant
// address space, so the compiler fetches them with scalar loads (1,545 floats at most: they stay
// in the scalar cache) and each v_fma_f32 takes its weight from an SGPR; the result is already in
// the lane that stores the action. Nothing here uses LDS. -ffp-contract=off (hipflags.mk) leaves
// the explicit fmaf calls alone and keeps the noise add a separate rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_sample.hpp"

namespace macm {

constexpr int kPolicyLogits = 9;  // MultiDiscrete([3, 3, 3]): head h at logits[3h + c]

// What the kernels take of a registered policy and of one rollout call (device pointers)
struct PolicyArgs {
  const float* params;  // W1[OD][H], b1[H], (W2[H][H], b2[H]), W3[H][9], b3[9]; 16-byte aligned
  const float* noise;   // [rows, 9] or NULL
  float* logits;        // [rows, 9] or NULL
  int32_t hidden;       // H: 16 or 32
  int32_t n_hidden;     // 1 or 2
};

using policy_cptr = const __attribute__((address_space(4))) float*;

// y[j] = b[j] + sum_k W[k][j] x[k] as the k-ordered fmaf chain; W, b wave-uniform
template <int IN, int OUT, bool RELU>
__device__ __forceinline__ void policy_layer(policy_cptr W, policy_cptr b, const float (&x)[IN], float (&y)[OUT]) {
#pragma unroll
  for (int j = 0; j < OUT; ++j) y[j] = b[j];
#pragma unroll
  for (int k = 0; k < IN; ++k) {
#pragma unroll
    for (int j = 0; j < OUT; ++j) y[j] = __builtin_fmaf(W[k * OUT + j], x[k], y[j]);
  }
  if constexpr (RELU) {
#pragma unroll
    for (int j = 0; j < OUT; ++j) y[j] = y[j] > 0.0f ? y[j] : 0.0f;
  }
}

// SMP (the sampled form, policy_sample.hpp): the noise is the draw sd's, not read; it is produced head
// by head after the logits are stored, when the MLP's activations are dead, and consumed at once by
// the running argmax
template <typename OT, int OD, int H, bool SMP = false>
__device__ __forceinline__ void policy_mlp_row_t(policy_cptr p, int n_hidden, const OT* __restrict__ o,
                                                 const float* __restrict__ noise, uint8_t* __restrict__ act,
                                                 float* __restrict__ logits, const SampleDraw& sd = SampleDraw{}) {
  float x[OD];
#pragma unroll
  for (int q = 0; q < OD; ++q) x[q] = (float)o[q];
  float h[H];
  policy_layer<OD, H, true>(p, p + OD * H, x, h);
  p += OD * H + H;
  if (n_hidden == 2) {  // wave-uniform
    float g[H];
    policy_layer<H, H, true>(p, p + H * H, h, g);
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = g[j];
    p += H * H + H;
  }
  float y[kPolicyLogits];
  policy_layer<H, kPolicyLogits, false>(p, p + H * kPolicyLogits, h, y);
  if (logits) {
#pragma unroll
    for (int j = 0; j < kPolicyLogits; ++j) logits[j] = y[j];
  }
  if constexpr (!SMP) {
    if (noise) {
#pragma unroll
      for (int j = 0; j < kPolicyLogits; ++j) y[j] = y[j] + noise[j];
    }
  }
#pragma unroll
  for (int hd = 0; hd < 3; ++hd) {
    if constexpr (SMP) {
      float g[3];
      gumbel_row(sd, hd, g);
#pragma unroll
      for (int c = 0; c < 3; ++c) y[3 * hd + c] = y[3 * hd + c] + g[c];
    }
    int best = 0;
    float bz = -__builtin_inff();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (y[3 * hd + c] > bz) {
        best = c;
        bz = y[3 * hd + c];
      }
    }
    act[hd] = (uint8_t)best;
  }
}

// o: the agent's obs row (od = 4 polar / 6 cartesian) as stored; noise / logits: its 9 floats or NULL;
// act: its 3 action bytes. M.params, M.hidden and M.n_hidden must be wave-uniform.
// SMP: the row draws its noise itself (sd; `noise` is not read)
template <typename OT, bool SMP = false>
__device__ __forceinline__ void policy_mlp_row(const PolicyArgs& M, int od, const OT* __restrict__ o,
                                               const float* __restrict__ noise, uint8_t* __restrict__ act,
                                               float* __restrict__ logits, const SampleDraw& sd = SampleDraw{}) {
  const policy_cptr p = (policy_cptr)(unsigned long long)M.params;
  if (od == 6) {
    if (M.hidden == 32)
      policy_mlp_row_t<OT, 6, 32, SMP>(p, M.n_hidden, o, noise, act, logits, sd);
    else
      policy_mlp_row_t<OT, 6, 16, SMP>(p, M.n_hidden, o, noise, act, logits, sd);
  } else {
    if (M.hidden == 32)
      policy_mlp_row_t<OT, 4, 32, SMP>(p, M.n_hidden, o, noise, act, logits, sd);
    else
      policy_mlp_row_t<OT, 4, 16, SMP>(p, M.n_hidden, o, noise, act, logits, sd);
  }
}

// The critic (include/macm.h, macm_value_mlp): a second MLP of the same arithmetic over the same obs
// row, with a trunk of its own and one output, V(obs). What the kernels take of a registered critic
// and of one rollout call (device pointers):
struct ValueArgs {
  const float* params;  // W1[OD][H], b1[H], (W2[H][H], b2[H]), W3[H][1], b3[1]; 16-byte aligned
  float* values;        // rollouts: [E, N], or [K + 1, E, N] with traj (row 0 is the caller's); NULL: not wanted
  float* boot;          // rollouts: [E, N], or [K, E, N] with traj; NULL: not wanted
  int32_t hidden;       // H: 16 or 32
  int32_t n_hidden;     // 1 or 2
};

template <typename OT, int OD, int H>
__device__ __forceinline__ float value_mlp_row_t(policy_cptr p, int n_hidden, const OT* __restrict__ o) {
  float x[OD];
#pragma unroll
  for (int q = 0; q < OD; ++q) x[q] = (float)o[q];
  float h[H];
  policy_layer<OD, H, true>(p, p + OD * H, x, h);
  p += OD * H + H;
  if (n_hidden == 2) {  // wave-uniform
    float g[H];
    policy_layer<H, H, true>(p, p + H * H, h, g);
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = g[j];
    p += H * H + H;
  }
  float y[1];
  policy_layer<H, 1, false>(p, p + H, h, y);
  return y[0];
}

// V of the agent's obs row o (od = 4 polar / 6 cartesian) as stored. V.params, V.hidden and V.n_hidden
// must be wave-uniform.
template <typename OT>
__device__ __forceinline__ float value_mlp_row(const ValueArgs& V, int od, const OT* __restrict__ o) {
  const policy_cptr p = (policy_cptr)(unsigned long long)V.params;
  if (od == 6) {
    if (V.hidden == 32) return value_mlp_row_t<OT, 6, 32>(p, V.n_hidden, o);
    return value_mlp_row_t<OT, 6, 16>(p, V.n_hidden, o);
  }
  if (V.hidden == 32) return value_mlp_row_t<OT, 4, 32>(p, V.n_hidden, o);
  return value_mlp_row_t<OT, 4, 16>(p, V.n_hidden, o);
}

// host side (C++ linkage, capi_learn.hip and capi_world.hip): the one-shot kernels over rows and the GAE kernel (policy.hip)
hipError_t launch_value_flock(const ValueArgs& V, const void* obs, bool obs_f64, int od, long long rows, float* values,
                              hipStream_t s);
// (host side) a GAE pass: [K, E, N] rewards, values and boot, [K, E] done flags
struct GaeShape {
  int n_steps;
  long long n_envs;
  int n_agents;
  float gamma, lambda;
};
hipError_t launch_gae(const float* reward, const float* values, const float* boot, const uint8_t* done,
                      const GaeShape& g, float* adv, float* ret, hipStream_t s);
hipError_t launch_policy_flock(const PolicyArgs& M, const void* obs, bool obs_f64, int od, long long rows,
                               uint8_t* act, hipStream_t s);
// launch_policy_flock with the draw inside: row r at decision S.decision (M.noise is not read)
hipError_t launch_policy_flock_sampled(const PolicyArgs& M, const SampleArgs& S, const void* obs, bool obs_f64, int od,
                                       long long rows, uint8_t* act, hipStream_t s);
// the noise decisions S.decision .. + n_dec - 1 draw for rows r < rows: noise [n_dec, rows, 9], and the raw
// words [n_dec, rows, 3, 4] (or NULL)
hipError_t launch_policy_noise(const SampleArgs& S, long long n_dec, long long rows, float* noise, uint32_t* words,
                               hipStream_t s);

// host side, policy_grad.hip: dL/dparams of either net (n_out = 9: the policy, 1: the critic) from dout
// [rows, n_out] (macm_policy_grad / macm_value_grad). One wave writes one partial [n_params] into the
// workspace, at most kGradMaxPartials of them; kGradMaxParams bounds n_params over the supported shapes.
constexpr int kGradMaxPartials = 2048;
// floats of a net's params: W1[od][h], b1[h], (W2[h][h], b2[h]), W3[h][n_out], b3[n_out]
constexpr int mlp_n_params(int od, int hidden, int n_hidden, int n_out) {
  return od * hidden + hidden + (n_hidden == 2 ? hidden * hidden + hidden : 0) + hidden * n_out + n_out;
}
constexpr int kGradMaxParams = mlp_n_params(6, 32, 2, kPolicyLogits);  // 1,577
long long mlp_grad_partials(long long rows);  // min(ceil(rows / 64), kGradMaxPartials)
// Either net as the gradient launches take it (host side; never a kernel parameter)
struct MlpNet {
  const float* params;
  int od, hidden, n_hidden, n_out;
  int n_params() const { return mlp_n_params(od, hidden, n_hidden, n_out); }
};
hipError_t launch_mlp_grad(const MlpNet& net, const void* obs, bool obs_f64, long long rows, const float* dout,
                           float* grad, float* workspace, hipStream_t s);

}  // namespace macm
