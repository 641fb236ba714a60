// f64_forms_probe.hip — test-only kernel for tests/test_gpu_f64_forms.py: the division that
// obs_atan2_core writes out on the device (macm_div_f32sums, csrc/macm_math.h) beside the
// compiler's own lowering of `/` on the same operands, one element per thread. Built by
// tests/probe/forms.mk with the product's HIPFLAGS, as the Makefile beside it builds macm_probe.hip.
//
// Entry point: device pointers and a count, launched on the null stream, synchronised; returns the
// HIP status (0 = hipSuccess), or -1 for a count the launch cannot take.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "macm_math.h"

namespace {

constexpr int kBlock = 256;

__global__ void k_div_forms(const double* num, const double* den, double* q_forms, double* q_plain, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  q_forms[i] = macm_div_f32sums(num[i], den[i]);
  q_plain[i] = num[i] / den[i];
}

}  // namespace

extern "C" int probe_div_forms(const double* num, const double* den, double* q_forms, double* q_plain, size_t n) {
  if (n == 0) return 0;
  if (n > (size_t)0x7fffffff) return -1;
  hipLaunchKernelGGL(k_div_forms, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, num, den, q_forms,
                     q_plain, n);
  const hipError_t launch = hipGetLastError();
  const hipError_t sync = hipDeviceSynchronize();
  return (int)(launch != hipSuccess ? launch : sync);
}
