// policy_grad.hpp — what the gradient kernels share (policy_grad.hip: the two MLPs; tdm_policy_grad.hip: the
// TDM set policy): the per-row backward of a layer, the weight gradient of a layer as an MFMA outer product
// over a tile's 64 rows, and the stores of a wave's partial. The layouts are policy_grad.hip's (its header
// comment): lane = row, operand images [64 rows][33] in LDS, one 32 x 32 accumulator block per layer.
#pragma once
#include "policy_mlp.hpp"

namespace macm {

using grad_f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kGradLds = 33;  // floats per row of an LDS operand image: 32 columns and one of padding

// d_prev[k] = a[k] > 0 ? sum_j W[k][j] d[j] : 0, the sum as the j-ordered fmaf chain from +0; W wave-uniform
template <int IN, int OUT>
__device__ __forceinline__ void grad_back_layer(policy_cptr W, const float (&a)[IN], const float (&d)[OUT],
                                                float (&dp)[IN]) {
#pragma unroll
  for (int k = 0; k < IN; ++k) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < OUT; ++j) s = __builtin_fmaf(W[k * OUT + j], d[j], s);
    dp[k] = a[k] > 0.0f ? s : 0.0f;
  }
}

// acc += a^T d over the tile's 64 rows: the lane's row of each operand into its LDS image, then 32 MFMAs
template <int IN, int OUT>
__device__ __forceinline__ void grad_outer(float* __restrict__ sA, float* __restrict__ sB, const float (&a)[IN],
                                           const float (&d)[OUT], grad_f32x16& acc, int lane) {
  static_assert(IN <= 32 && OUT <= 32, "one 32 x 32 block");
  __syncthreads();  // the reads of the images' last use are done
#pragma unroll
  for (int k = 0; k < IN; ++k) sA[lane * kGradLds + k] = a[k];
#pragma unroll
  for (int j = 0; j < OUT; ++j) sB[lane * kGradLds + j] = d[j];
  __syncthreads();
  const int at = (lane >> 5) * kGradLds + (lane & 31);
#pragma unroll
  for (int s = 0; s < 32; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[at + 2 * s * kGradLds], sB[at + 2 * s * kGradLds], acc, 0, 0, 0);
}

// The [IN x OUT] corner of a 32 x 32 accumulator block into dst[i * OUT + j]; register g of lane l holds
// row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31
template <int IN, int OUT>
__device__ __forceinline__ void grad_store_block(const grad_f32x16& acc, float* __restrict__ dst, int lane) {
  const int j = lane & 31;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int i = (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
    if (i < IN && j < OUT) dst[i * OUT + j] = acc[g];
  }
}

// dst[j] = sum over lanes (in lane order) of b[j], through an LDS image
template <int OUT>
__device__ __forceinline__ void grad_store_bias(float* __restrict__ sm, const float (&b)[OUT], float* __restrict__ dst,
                                                int lane) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < OUT; ++j) sm[lane * kGradLds + j] = b[j];
  __syncthreads();
  if (lane < OUT) {
    float s = 0.0f;
    for (int r = 0; r < 64; ++r) s = s + sm[r * kGradLds + lane];
    dst[lane] = s;
  }
}

}  // namespace macm
