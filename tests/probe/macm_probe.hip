// macm_probe.hip — test-only kernels around the step's exact-arithmetic and wave primitives
// (tests/test_gpu_primitives.py). Each kernel calls ONE function of the product headers, one
// element per thread, reading its inputs from and writing its results to device arrays; no
// arithmetic of the headers is restated here. Built by tests/probe/Makefile with the product's
// HIPFLAGS: the point is to test the code the product compiles.
//
// Entry points: device pointers and a count, launched on the null stream, synchronised; the return
// value is the HIP status (0 = hipSuccess), or -1 for a count / block size the kernel cannot take.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "flock_common.hpp"
#include "flock_spill.hpp"
#include "macm_math.h"

using namespace macm;

namespace {

constexpr int kBlock = 256;

// ---- one element per thread --------------------------------------------------------------------

__global__ void k_rcp_rn(const float* x, float* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rcp_rn(x[i]);
}

__global__ void k_sqrt_rn(const float* x, float* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sqrt_rn(x[i]);
}

template <typename OT>
__global__ void k_obs_sqrt(const float* x, double* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = obs_sqrt<OT>(x[i]);
}

__global__ void k_div_by_invariant(const float* num, const float* K, float* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = div_by_invariant(num[i], K[i]);
}

__global__ void k_act_trig(const float* a, double* out4, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s0, c0, s1, c1;
  act_trig(a[i], &s0, &c0, &s1, &c1);
  out4[4 * i + 0] = s0;
  out4[4 * i + 1] = c0;
  out4[4 * i + 2] = s1;
  out4[4 * i + 3] = c1;
}

__global__ void k_obs_atan2(const double* y, const double* x, double* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = obs_atan2(y[i], x[i]);
}

// the other agent's view of a TDM pair: the core of (|x|, |y|) finished with the signs of (-y, -x)
__global__ void k_obs_atan2_split_neg(const double* y, const double* x, double* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = obs_atan2_finish(obs_atan2_core(fabs(x[i]), fabs(y[i])), -y[i], -x[i]);
}

// ---- wave and block primitives: blocks of whole waves, every lane active ---------------------------

__global__ void k_wave_prefix_max(const int* in, int* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[i] = wave_prefix_max(in[i]);
}

__global__ void k_wave_prefix_sum(const int* in, int* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[i] = wave_prefix_sum(in[i]);
}

__global__ void k_wave_max(const int* in, int* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[i] = wave_max(in[i]);
}

__global__ void k_wave_pairwise_sum(const double* in, double* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[i] = wave_pairwise_sum(in[i]);
}

__global__ void k_block_pairwise_sum(const double* in, double* out) {  // out: one value per block
  __shared__ double s_tmp[16];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double v = block_pairwise_sum(in[i], s_tmp);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__global__ void k_block_scan_excl(const int* in, int* excl_out, int* total_out) {
  __shared__ int s_scan[32];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int excl;
  const int total = spill::block_scan_excl(in[i], excl, s_scan);
  excl_out[i] = excl;
  total_out[i] = total;
}

int finish() {
  const hipError_t launch = hipGetLastError();
  const hipError_t sync = hipDeviceSynchronize();
  return (int)(launch != hipSuccess ? launch : sync);
}

unsigned grid_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// whole waves, at most 16 of them, and n a whole number of blocks
bool blocks_ok(size_t n, int block) { return block >= 64 && block <= 1024 && block % 64 == 0 && n % (size_t)block == 0; }

}  // namespace

#define PROBE_ELEMENTWISE(kernel, ...)                                \
  if (n == 0) return 0;                                               \
  if (n > (size_t)0x7fffffff) return -1;                              \
  hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(kBlock), 0, 0, __VA_ARGS__, n); \
  return finish();

#define PROBE_BLOCKS(kernel, ...)                                     \
  if (n == 0) return 0;                                               \
  if (!blocks_ok(n, block) || n > (size_t)0x7fffffff) return -1;      \
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n / (size_t)block)), dim3(block), 0, 0, __VA_ARGS__); \
  return finish();

extern "C" {

int probe_rcp_rn(const float* x, float* out, size_t n) { PROBE_ELEMENTWISE(k_rcp_rn, x, out) }
int probe_sqrt_rn(const float* x, float* out, size_t n) { PROBE_ELEMENTWISE(k_sqrt_rn, x, out) }
int probe_obs_sqrt_f32(const float* x, double* out, size_t n) { PROBE_ELEMENTWISE(k_obs_sqrt<float>, x, out) }
int probe_obs_sqrt_f64(const float* x, double* out, size_t n) { PROBE_ELEMENTWISE(k_obs_sqrt<double>, x, out) }
int probe_div_by_invariant(const float* num, const float* K, float* out, size_t n) {
  PROBE_ELEMENTWISE(k_div_by_invariant, num, K, out)
}
int probe_act_trig(const float* a, double* out4, size_t n) { PROBE_ELEMENTWISE(k_act_trig, a, out4) }
int probe_obs_atan2(const double* y, const double* x, double* out, size_t n) {
  PROBE_ELEMENTWISE(k_obs_atan2, y, x, out)
}
int probe_obs_atan2_split_neg(const double* y, const double* x, double* out, size_t n) {
  PROBE_ELEMENTWISE(k_obs_atan2_split_neg, y, x, out)
}

// n threads in blocks of `block` (a multiple of 64, n a multiple of block)
int probe_wave_prefix_max(const int* in, int* out, size_t n, int block) { PROBE_BLOCKS(k_wave_prefix_max, in, out) }
int probe_wave_prefix_sum(const int* in, int* out, size_t n, int block) { PROBE_BLOCKS(k_wave_prefix_sum, in, out) }
int probe_wave_max(const int* in, int* out, size_t n, int block) { PROBE_BLOCKS(k_wave_max, in, out) }
int probe_wave_pairwise_sum(const double* in, double* out, size_t n, int block) {
  PROBE_BLOCKS(k_wave_pairwise_sum, in, out)
}
// out: n / block values, one per block
int probe_block_pairwise_sum(const double* in, double* out, size_t n, int block) {
  PROBE_BLOCKS(k_block_pairwise_sum, in, out)
}
// excl_out, total_out: n values each (every thread's view of its block's total)
int probe_block_scan_excl(const int* in, int* excl_out, int* total_out, size_t n, int block) {
  PROBE_BLOCKS(k_block_scan_excl, in, excl_out, total_out)
}

}  // extern "C"
