// ppo_loss.hip — the PPO loss on rows that are already in memory (include/macm.h): macm_policy_logp, the
// log-probability of the taken actions from stored logits, and macm_ppo_loss, from logits and values to
// dL/dlogits, dL/dvalue and the statistics in one pass. The row arithmetic is ppo_row.hpp's.
//
// One thread per row, grid-stride with 64-bit row indices: a wave's 64 logit rows are 2,304 contiguous
// bytes, so its nine loads (and stores) of one float per lane use full cache lines between them. About
// 90 B in and 40 B out per row against some 600 float64 operations: bandwidth-bound.
//
// Statistics without atomics: a lane sums its rows' terms in float64; a block's lanes are summed wave by
// wave in lane order and the four wave sums in order (LDS); block b writes partial b to the workspace.
// ppo_stats_kernel sums the partials in index order within 64 contiguous runs and then the run sums in
// order, and turns the sums into stats[8]. The grid is a function of `rows` alone, so the same inputs
// give the same bits on every call and stream.
//
// macm_adv_moments (below the stats kernel): the mean and unbiased std of a minibatch's advantages, read
// through the same index list as macm_ppo_grad_rows, with the same grid and association of the sums.
#include "ppo_row.hpp"

namespace macm {

__global__ __launch_bounds__(kPpoBlock) void policy_logp_kernel(const float* __restrict__ logits,
                                                                const uint8_t* __restrict__ actions, long long rows,
                                                                float* __restrict__ logp, float* __restrict__ entropy) {
  const long long stride = (long long)gridDim.x * kPpoBlock;
  for (long long r = (long long)blockIdx.x * kPpoBlock + threadIdx.x; r < rows; r += stride) {
    float z[9];
    uint8_t a[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) z[q] = logits[r * 9 + q];
#pragma unroll
    for (int h = 0; h < 3; ++h) a[h] = actions[r * 3 + h];
    double p[9], lp[9], Hh[3];
    logp[r] = (float)ppo_logp_row(z, a, p, lp, Hh);
    if (entropy) entropy[r] = (float)((Hh[0] + Hh[1]) + Hh[2]);
  }
}

__global__ __launch_bounds__(kPpoBlock) void ppo_loss_kernel(const PpoLossArgs A, long long rows) {
  __shared__ double sm[kPpoVl + 1][kPpoBlock];
  __shared__ double wave[kPpoVl + 1][kPpoBlock / 64];
  const int tid = threadIdx.x;
  const double k = (A.scale ? (double)A.scale[0] : 1.0) / (double)rows;
  double st[kPpoVl + 1];
#pragma unroll
  for (int q = 0; q <= kPpoVl; ++q) st[q] = 0.0;
  const long long stride = (long long)gridDim.x * kPpoBlock;
  for (long long r = (long long)blockIdx.x * kPpoBlock + tid; r < rows; r += stride) {
    if (A.logits) {
      float z[9], d[9];
      uint8_t a[3];
#pragma unroll
      for (int q = 0; q < 9; ++q) z[q] = A.logits[r * 9 + q];
#pragma unroll
      for (int h = 0; h < 3; ++h) a[h] = A.actions[r * 3 + h];
      PpoPolicyTerms T;
      ppo_policy_row(z, a, A.old_logp[r], A.adv[r], A.cfg, k, d, T);
      st[kPpoPl] = st[kPpoPl] + T.pl;
      st[kPpoH] = st[kPpoH] + T.H;
      st[kPpoKl] = st[kPpoKl] + T.kl;
      st[kPpoClipped] = st[kPpoClipped] + T.clipped;
      st[kPpoRatioMax] = T.ratio > st[kPpoRatioMax] ? T.ratio : st[kPpoRatioMax];
      if (A.dlogits) {
#pragma unroll
        for (int q = 0; q < 9; ++q) A.dlogits[r * 9 + q] = d[q];
      }
    }
    if (A.values) {
      double vl;
      const float dv = ppo_value_row(A.values[r], A.ret[r], A.old_values != nullptr,
                                     A.old_values ? A.old_values[r] : 0.0f, A.cfg, k, vl);
      st[kPpoVl] = st[kPpoVl] + vl;
      if (A.dvalues) A.dvalues[r] = dv;
    }
  }
  if (!A.part) return;  // (block-uniform)
#pragma unroll
  for (int q = 0; q <= kPpoVl; ++q) sm[q][tid] = st[q];
  __syncthreads();
  if (tid < (kPpoVl + 1) * (kPpoBlock / 64)) {  // thread (term q, wave w): the wave's lanes in lane order
    const int q = tid / (kPpoBlock / 64), w = tid % (kPpoBlock / 64);
    double s = 0.0;
    for (int l = 0; l < 64; ++l) {
      const double t = sm[q][w * 64 + l];
      s = q == kPpoRatioMax ? (t > s ? t : s) : s + t;
    }
    wave[q][w] = s;
  }
  __syncthreads();
  if (tid <= kPpoVl) {
    double s = 0.0;
    for (int w = 0; w < kPpoBlock / 64; ++w) {
      const double t = wave[tid][w];
      s = tid == kPpoRatioMax ? (t > s ? t : s) : s + t;
    }
    A.part[(size_t)blockIdx.x * kPpoStatSlots + tid] = s;
  }
}

// stats = {loss, policy_loss, value_loss, entropy, approx_kl, clip_frac, ratio_max, rows}. Thread (run g,
// term q) sums the g-th of 64 contiguous runs of the partials in index order, then thread (0, q) the 64 run
// sums in order; thread 0 combines them.
constexpr int kPpoRuns = 64;
__global__ __launch_bounds__(kPpoRuns * kPpoStatSlots) void ppo_stats_kernel(const double* __restrict__ part, int n_part,
                                                                             long long rows, const PpoCfg cfg,
                                                                             int has_policy, int has_value,
                                                                             double* __restrict__ stats) {
  __shared__ double run[kPpoStatSlots][kPpoRuns];
  __shared__ double tot[kPpoStatSlots];
  const int q = threadIdx.x & (kPpoStatSlots - 1), g = threadIdx.x / kPpoStatSlots;
  const bool live = q < kPpoPolicyTerms ? has_policy != 0 : (q == kPpoVl && has_value != 0);
  const int per = (n_part + kPpoRuns - 1) / kPpoRuns;
  const int lo = g * per, hi = lo + per < n_part ? lo + per : n_part;
  double s = 0.0;
  if (live) {
#pragma unroll 4
    for (int i = lo; i < hi; ++i) {
      const double t = part[(size_t)i * kPpoStatSlots + q];
      s = q == kPpoRatioMax ? (t > s ? t : s) : s + t;
    }
  }
  run[q][g] = s;
  __syncthreads();
  if (g == 0) {
    double a = 0.0;
    for (int i = 0; i < kPpoRuns; ++i) {
      const double t = run[q][i];
      a = q == kPpoRatioMax ? (t > a ? t : a) : a + t;
    }
    tot[q] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)rows;
    const double pl = tot[kPpoPl] / n, vl = tot[kPpoVl] / n, H = tot[kPpoH] / n;
    stats[0] = (pl + (double)cfg.vf_coef * vl) - (double)cfg.ent_coef * H;
    stats[1] = pl;
    stats[2] = vl;
    stats[3] = H;
    stats[4] = tot[kPpoKl] / n;
    stats[5] = tot[kPpoClipped] / n;
    stats[6] = tot[kPpoRatioMax];
    stats[7] = n;
  }
}

// ---- macm_adv_moments: mean and unbiased std of x[index[r]] in two passes, four small launches ------------
// adv_sum_kernel<0> sums x and counts the positions that count, adv_finish_kernel<0> writes out[0] = mean and
// out[3] = n; adv_sum_kernel<1> sums (x - mean)^2 with that mean, adv_finish_kernel<1> writes out[2] = std and
// out[1] = rstd. The grid and the sums' association are ppo_loss_kernel's: lane-local over the grid's stride,
// a wave's lanes in lane order, the block's four waves in order, partial b by block b; the finish kernels sum
// the partials in index order within 64 contiguous runs and then the run sums in order. All float64, each
// operation rounded once; a position whose source row is outside [0, n_src) is skipped before x is addressed.
template <int PASS>
__global__ __launch_bounds__(kPpoBlock) void adv_sum_kernel(const float* __restrict__ x,
                                                            const int32_t* __restrict__ index, long long n_src,
                                                            long long rows, const double* __restrict__ out,
                                                            double* __restrict__ part) {
  __shared__ double sm[2][kPpoBlock];
  __shared__ double wave[2][kPpoBlock / 64];
  const int tid = threadIdx.x;
  const double mean = PASS ? out[0] : 0.0;
  double a = 0.0, n = 0.0;
  const long long stride = (long long)gridDim.x * kPpoBlock;
  for (long long r = (long long)blockIdx.x * kPpoBlock + tid; r < rows; r += stride) {
    long long s = r;
    if (index) {  // (block-uniform)
      s = (long long)index[r];
      if ((unsigned long long)s >= (unsigned long long)n_src) continue;
    }
    const double v = (double)x[s];
    if (PASS == 0) {
      a = a + v;
      n = n + 1.0;
    } else {
      const double d = v - mean;
      a = a + d * d;
    }
  }
  sm[0][tid] = a;
  sm[1][tid] = n;
  __syncthreads();
  if (tid < 2 * (kPpoBlock / 64)) {  // thread (term q, wave w): the wave's lanes in lane order
    const int q = tid / (kPpoBlock / 64), w = tid % (kPpoBlock / 64);
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s = s + sm[q][w * 64 + l];
    wave[q][w] = s;
  }
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int w = 0; w < kPpoBlock / 64; ++w) s = s + wave[tid][w];
    part[(size_t)blockIdx.x * 2 + tid] = s;
  }
}

constexpr int kAdvRuns = 64;
template <int PASS>
__global__ __launch_bounds__(2 * kAdvRuns) void adv_finish_kernel(const double* __restrict__ part, int n_part,
                                                                  double eps, double* __restrict__ out) {
  __shared__ double run[2][kAdvRuns];
  const int q = threadIdx.x & 1, g = threadIdx.x >> 1;
  const int per = (n_part + kAdvRuns - 1) / kAdvRuns;
  const int lo = g * per, hi = lo + per < n_part ? lo + per : n_part;
  double s = 0.0;
  if (PASS == 0 || q == 0) {  // (the second pass has no count)
#pragma unroll 4
    for (int i = lo; i < hi; ++i) s = s + part[(size_t)i * 2 + q];
  }
  run[q][g] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, n = 0.0;
    for (int i = 0; i < kAdvRuns; ++i) {
      a = a + run[0][i];
      n = n + run[1][i];
    }
    if (PASS == 0) {
      out[0] = n > 0.0 ? a / n : 0.0;
      out[3] = n;
    } else {
      n = out[3];
      const double sd = sqrt(n > 1.0 ? a / (n - 1.0) : 0.0);
      out[1] = 1.0 / (sd + eps);
      out[2] = sd;
    }
  }
}

hipError_t launch_adv_moments(const float* x, const int32_t* index, long long n_src, long long rows, double eps,
                              double* out, double* part, hipStream_t s) {
  const int P = rows > 0 ? (int)ppo_loss_partials(rows) : 0;  // rows = 0: the finish kernels alone, over no partials
  const dim3 grid((unsigned)P), block(kPpoBlock), one(1), fin(2 * kAdvRuns);
  if (P > 0) hipLaunchKernelGGL(adv_sum_kernel<0>, grid, block, 0, s, x, index, n_src, rows, out, part);
  hipLaunchKernelGGL(adv_finish_kernel<0>, one, fin, 0, s, part, P, eps, out);
  if (P > 0) hipLaunchKernelGGL(adv_sum_kernel<1>, grid, block, 0, s, x, index, n_src, rows, out, part);
  hipLaunchKernelGGL(adv_finish_kernel<1>, one, fin, 0, s, part, P, eps, out);
  return hipGetLastError();
}

long long ppo_loss_partials(long long rows) {
  const long long blocks = (rows + kPpoBlock - 1) / kPpoBlock;
  return blocks < kPpoMaxBlocks ? blocks : kPpoMaxBlocks;
}

hipError_t launch_policy_logp(const float* logits, const uint8_t* actions, long long rows, float* logp, float* entropy,
                              hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(policy_logp_kernel, dim3((unsigned)ppo_loss_partials(rows)), dim3(kPpoBlock), 0, s, logits,
                     actions, rows, logp, entropy);
  return hipGetLastError();
}

hipError_t launch_ppo_loss(const PpoLossArgs& A, long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ppo_loss_kernel, dim3((unsigned)ppo_loss_partials(rows)), dim3(kPpoBlock), 0, s, A, rows);
  return hipGetLastError();
}

hipError_t launch_ppo_stats(const double* part, int n_part, long long rows, const PpoCfg& cfg, bool has_policy,
                            bool has_value, double* stats, hipStream_t s) {
  hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(kPpoRuns * kPpoStatSlots), 0, s, part, n_part, rows, cfg,
                     has_policy ? 1 : 0, has_value ? 1 : 0, stats);
  return hipGetLastError();
}

}  // namespace macm
