// policy_grad.hip — parameter gradients of the two MLPs (macm_policy_grad / macm_value_grad): from
// dL/dout of every row to dL/dparams, one launch per net plus a small reduction.
//
// The definition (include/macm.h): the forward is policy_mlp.hpp's, bit for bit; with a_0 the float32
// obs row, a_l the stored (post-relu) activation of hidden layer l and d_L = dout, from the last layer
// to the first
//   gW_l[k][j] = sum_r a_{l-1}[r][k] d_l[r][j]     gb_l[j] = sum_r d_l[r][j]
//   d_{l-1}[r][k] = a_{l-1}[r][k] > 0 ? sum_j W_l[k][j] d_l[r][j] : 0
// all float32. The sums' association is this file's, fixed by `rows` alone: no atomics anywhere.
//
// Per-row part (VALU): one wave per block, lane = row, tiles of 64 rows. The forward is recomputed with
// policy_layer and scalar-loaded weights exactly as policy_mlp_row_t does, x, h1, h2 stay in registers;
// each d_{l-1}[k] is the j-ordered fmaf chain from +0 over W_l[k][0..OUT), whose operands are again
// wave-uniform (contiguous in j: wide scalar loads). Nothing per row goes to global memory.
//
// Weight gradients (MFMA): gW_l = A_{l-1}^T [in x 64] · D_l [64 x out], contracted over the tile's rows
// with v_mfma_f32_32x32x2_f32 (exact f32, the k-ordered fmaf chain). Lane l supplies A[i = l & 31][k = l >> 5]
// and B[k = l >> 5][j = l & 31], so both operands are read from row-major LDS images [64 rows][33] at
// [row 2s + (l >> 5)][l & 31] for s = 0..31: 32 MFMAs per layer and tile into 16 accumulator registers that
// live across all of the wave's tiles. The images are written lane = row (stride 33: conflict-free) and
// only their first `in` / `out` columns; the MFMA reads all 32, and what it reads past them lands in
// output rows / columns that are never stored (row i of the product depends on A's column i alone, column
// j on B's column j alone). So H = 16, the 9 or 1 outputs and the 4 or 6 inputs use the 32 x 32 tile
// partly empty rather than 16x16x4: one code path, and the MFMA pipe is not what limits this kernel.
//
// Bias gradients: gb_1 rides in the first layer's product as a ones column behind x (in + 1 <= 7 columns
// of 32). The other layers' A operand may be full (H = 32), so gb_2 and gb_3 are lane-local float32 sums
// over the wave's tiles, reduced once per wave at the end through LDS in lane order.
//
// Cross-wave reduction: P = min(tiles, kGradMaxPartials) waves; wave w takes tiles w, w + P, w + 2P, ...
// (64-bit row indices) and writes one partial [n_params] to the caller's workspace. mlp_grad_reduce_kernel
// sums the P partials per parameter in index order in float64 (four contiguous runs, then the four run
// sums in order) and rounds once. A tail lane past `rows` loads nothing and carries x = 0, dout = 0: every
// d of it is an exact zero and so is each of its products.
//
// Loss-to-gradient launches (macm_ppo_grad): the same body with DoutPpo in the place of DoutMem. The forward
// goes on through the last layer (policy_layer with b3: the bits of macm_policy_mlp / macm_value_mlp) and
// d_L of the lane's row is ppo_row.hpp's ppo_policy_row / ppo_value_row of those outputs, so neither the
// logits nor dL/dlogits exist in memory; everything after d_L is the code above. The row's stat terms are
// lane-local float64 sums over the wave's tiles, reduced once per wave through LDS in lane order into the
// wave's stat partial. A tail lane's d_L is zero and it adds nothing to the stats.
//
// Row-indexed launches (macm_ppo_grad_rows): the same body with DoutPpoRows, in kernels of their own. Lane l
// of tile t is position r = 64 t + l as before and reads source row s = index[r] of obs and of the loss's
// inputs; a position whose s is outside [0, n_src) becomes a tail lane before anything is addressed with
// it. The advantage is normalised in float64 as it is loaded. Tiles, waves, partials and every sum stay
// functions of the position: the outputs have the bits of macm_ppo_grad on gathered copies.
//
// grad_back_layer, grad_outer, grad_store_block and grad_store_bias live in policy_grad.hpp, which
// tdm_policy_grad.hip shares.
#include <type_traits>

#include "policy_grad.hpp"
#include "ppo_row.hpp"

namespace macm {

// Where d_L comes from: the caller's dout [rows, NOUT], or the PPO loss of the forward's own outputs
struct DoutMem {
  static constexpr bool kMem = true;  // (the body's dout argument)
  static constexpr bool kRows = false;
};
struct DoutPpo {
  static constexpr bool kMem = false;
  static constexpr bool kRows = false;
  PpoGradArgs G;
};
// ... of source row index[r] in the place of row r, with the advantage normalised on the way in
struct DoutPpoRows {
  static constexpr bool kMem = false;
  static constexpr bool kRows = true;
  PpoGradArgs G;
  PpoRowsArgs R;
};
using norm_cptr = const __attribute__((address_space(4))) double*;  // adv_norm: wave-uniform scalar loads

// d3 and the stat terms of the lane's row r (where the lane is live) from the last hidden activation: the
// output layer, then the loss
template <int H, int NOUT, typename Src>
__device__ __forceinline__ void grad_ppo_dout(policy_cptr W3, policy_cptr b3, const float (&h)[H], long long r,
                                              bool live, const Src& src, float (&d3)[NOUT],
                                              double (&st)[kPpoPolicyTerms]) {
  const PpoGradArgs& G = src.G;
  float y[NOUT];
  policy_layer<H, NOUT, false>(W3, b3, h, y);
  if (live) {
    if constexpr (NOUT == kPolicyLogits) {
      uint8_t a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = G.actions[r * 3 + q];
      const float old_logp = G.old_logp[r];
      float adv = G.adv[r];
      if constexpr (Src::kRows) {
        if (src.R.norm) {  // (wave-uniform)
          const norm_cptr nm = (norm_cptr)(unsigned long long)src.R.norm;
          adv = (float)(((double)adv - nm[0]) * nm[1]);
        }
      }
      PpoPolicyTerms T;
      ppo_policy_row(y, a, old_logp, adv, G.cfg, G.k, d3, T);
      st[kPpoPl] = st[kPpoPl] + T.pl;
      st[kPpoH] = st[kPpoH] + T.H;
      st[kPpoKl] = st[kPpoKl] + T.kl;
      st[kPpoClipped] = st[kPpoClipped] + T.clipped;
      st[kPpoRatioMax] = T.ratio > st[kPpoRatioMax] ? T.ratio : st[kPpoRatioMax];
    } else {
      double vl;
      d3[0] = ppo_value_row(y[0], G.ret[r], G.old_values != nullptr, G.old_values ? G.old_values[r] : 0.0f, G.cfg,
                            G.k, vl);
      st[0] = st[0] + vl;
    }
  }
}

template <typename OT, int OD, int H, int NH, int NOUT, typename Src = DoutMem>
__device__ __forceinline__ void mlp_grad_body(policy_cptr p, const OT* __restrict__ obs, long long rows,
                                              const float* __restrict__ dout, float* __restrict__ part,
                                              float* __restrict__ sA, float* __restrict__ sB, const Src& src = Src{}) {
  const int lane = threadIdx.x;
  const long long tiles = (rows + 63) >> 6;
  const policy_cptr W1 = p, b1 = W1 + OD * H;
  const policy_cptr W2 = b1 + H, b2 = W2 + H * H;  // (NH == 2)
  const policy_cptr W3 = NH == 2 ? b2 + H : b1 + H;  // (DoutMem: b3 is not read, the forward stops at the last hidden layer)
  [[maybe_unused]] const policy_cptr b3 = W3 + H * NOUT;
  [[maybe_unused]] double st[kPpoPolicyTerms];  // DoutPpo: the wave's stat terms (the critic: st[0] alone)
  if constexpr (!Src::kMem) {
#pragma unroll
    for (int q = 0; q < kPpoPolicyTerms; ++q) st[q] = 0.0;
  }
  grad_f32x16 acc1, acc2, acc3;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc1[g] = acc2[g] = acc3[g] = 0.0f;
  float bs2[H], bs3[NOUT];
#pragma unroll
  for (int j = 0; j < H; ++j) bs2[j] = 0.0f;
#pragma unroll
  for (int j = 0; j < NOUT; ++j) bs3[j] = 0.0f;

  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    long long r = t * 64 + lane;  // the lane's position, and from here on the row it reads
    bool live = r < rows;
    if constexpr (Src::kRows) {
      if (src.R.index) {  // (wave-uniform) a source row outside the arrays: a tail lane, never an address
        r = live ? (long long)src.R.index[r] : -1;
        live = (unsigned long long)r < (unsigned long long)src.R.n_src;
      }
    }
    float x[OD], d3[NOUT];
#pragma unroll
    for (int q = 0; q < OD; ++q) x[q] = 0.0f;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) d3[j] = 0.0f;
    if (live) {
#pragma unroll
      for (int q = 0; q < OD; ++q) x[q] = (float)obs[r * OD + q];
      if constexpr (Src::kMem) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) d3[j] = dout[r * NOUT + j];
      }
    }
    float h1[H], dtop[H];
    policy_layer<OD, H, true>(W1, b1, x, h1);
    if constexpr (NH == 2) {
      float h2[H];
      policy_layer<H, H, true>(W2, b2, h1, h2);
      if constexpr (!Src::kMem) grad_ppo_dout<H, NOUT>(W3, b3, h2, r, live, src, d3, st);
      grad_outer<H, NOUT>(sA, sB, h2, d3, acc3, lane);
      grad_back_layer<H, NOUT>(W3, h2, d3, dtop);
    } else {
      if constexpr (!Src::kMem) grad_ppo_dout<H, NOUT>(W3, b3, h1, r, live, src, d3, st);
      grad_outer<H, NOUT>(sA, sB, h1, d3, acc3, lane);
      grad_back_layer<H, NOUT>(W3, h1, d3, dtop);
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) bs3[j] = bs3[j] + d3[j];
    float xs[OD + 1];  // x and the ones column that sums d1 into gb_1
#pragma unroll
    for (int q = 0; q < OD; ++q) xs[q] = x[q];
    xs[OD] = 1.0f;
    if constexpr (NH == 2) {
      grad_outer<H, H>(sA, sB, h1, dtop, acc2, lane);
#pragma unroll
      for (int j = 0; j < H; ++j) bs2[j] = bs2[j] + dtop[j];
      float d1[H];
      grad_back_layer<H, H>(W2, h1, dtop, d1);
      grad_outer<OD + 1, H>(sA, sB, xs, d1, acc1, lane);
    } else {
      grad_outer<OD + 1, H>(sA, sB, xs, dtop, acc1, lane);
    }
  }

  // the wave's partial, in the layout of params: rows 0..OD-1 of the first block are W1, row OD is b1
  grad_store_block<OD + 1, H>(acc1, part, lane);
  float* o = part + OD * H + H;
  if constexpr (NH == 2) {
    grad_store_block<H, H>(acc2, o, lane);
    grad_store_bias<H>(sA, bs2, o + H * H, lane);
    o += H * H + H;
  }
  grad_store_block<H, NOUT>(acc3, o, lane);
  grad_store_bias<NOUT>(sB, bs3, o + H * NOUT, lane);

  if constexpr (!Src::kMem) {  // the wave's stat partial: term q's 64 lane sums in lane order, by lane q
    if (!src.G.stat) return;  // (wave-uniform: the caller wants no stats)
    constexpr int NS = NOUT == kPolicyLogits ? kPpoPolicyTerms : 1;
    double* const sd = reinterpret_cast<double*>(sA);  // (the kernel aligns sA; 5 x 64 doubles of its 8,448 bytes)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NS; ++q) sd[q * 64 + lane] = st[q];
    __syncthreads();
    if (lane < NS) {
      double s = 0.0;
      for (int l = 0; l < 64; ++l) {
        const double t = sd[lane * 64 + l];
        s = (NOUT == kPolicyLogits && lane == kPpoRatioMax) ? (t > s ? t : s) : s + t;
      }
      src.G.stat[(size_t)blockIdx.x * kPpoStatSlots + (NOUT == kPolicyLogits ? lane : kPpoVl)] = s;
    }
  }
}

// One wave per block; block b writes partial b. od, hidden and n_hidden are kernel arguments: the branches
// are wave-uniform, each body fully unrolled, as policy_mlp_row's.
template <typename OT, int NOUT>
__global__ __launch_bounds__(64) void mlp_grad_kernel(const float* __restrict__ params, int od, int hidden,
                                                      int n_hidden, const OT* __restrict__ obs, long long rows,
                                                      const float* __restrict__ dout, float* __restrict__ partials,
                                                      int n_params) {
  __shared__ float sA[64 * kGradLds], sB[64 * kGradLds];
  const policy_cptr p = (policy_cptr)(unsigned long long)params;
  float* const part = partials + (size_t)blockIdx.x * n_params;
#define MACM_GRAD_BODY(OD_, H_, NH_) mlp_grad_body<OT, OD_, H_, NH_, NOUT>(p, obs, rows, dout, part, sA, sB)
  if (od == 6) {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 32, 2); else MACM_GRAD_BODY(6, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 16, 2); else MACM_GRAD_BODY(6, 16, 1);
    }
  } else {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 32, 2); else MACM_GRAD_BODY(4, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 16, 2); else MACM_GRAD_BODY(4, 16, 1);
    }
  }
#undef MACM_GRAD_BODY
}

// The same launch with the PPO loss in the place of dout (macm_ppo_grad); block b also writes stat partial b
template <typename OT, int NOUT>
__global__ __launch_bounds__(64) void mlp_ppo_grad_kernel(const float* __restrict__ params, int od, int hidden,
                                                          int n_hidden, const OT* __restrict__ obs, long long rows,
                                                          const PpoGradArgs G, float* __restrict__ partials,
                                                          int n_params) {
  __shared__ __attribute__((aligned(16))) float sA[64 * kGradLds];
  __shared__ float sB[64 * kGradLds];
  const policy_cptr p = (policy_cptr)(unsigned long long)params;
  float* const part = partials + (size_t)blockIdx.x * n_params;
  const DoutPpo src{G};
#define MACM_GRAD_BODY(OD_, H_, NH_) \
  mlp_grad_body<OT, OD_, H_, NH_, NOUT, DoutPpo>(p, obs, rows, nullptr, part, sA, sB, src)
  if (od == 6) {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 32, 2); else MACM_GRAD_BODY(6, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 16, 2); else MACM_GRAD_BODY(6, 16, 1);
    }
  } else {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 32, 2); else MACM_GRAD_BODY(4, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 16, 2); else MACM_GRAD_BODY(4, 16, 1);
    }
  }
#undef MACM_GRAD_BODY
}

// The same launch again with the rows read through an index and the advantage normalised on the way in
// (macm_ppo_grad_rows): kernels of their own, so that the two above stay what they are
template <typename OT, int NOUT>
__global__ __launch_bounds__(64) void mlp_ppo_grad_rows_kernel(const float* __restrict__ params, int od, int hidden,
                                                               int n_hidden, const OT* __restrict__ obs,
                                                               long long rows, const PpoGradArgs G,
                                                               const PpoRowsArgs R, float* __restrict__ partials,
                                                               int n_params) {
  __shared__ __attribute__((aligned(16))) float sA[64 * kGradLds];
  __shared__ float sB[64 * kGradLds];
  const policy_cptr p = (policy_cptr)(unsigned long long)params;
  float* const part = partials + (size_t)blockIdx.x * n_params;
  const DoutPpoRows src{G, R};
#define MACM_GRAD_BODY(OD_, H_, NH_) \
  mlp_grad_body<OT, OD_, H_, NH_, NOUT, DoutPpoRows>(p, obs, rows, nullptr, part, sA, sB, src)
  if (od == 6) {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 32, 2); else MACM_GRAD_BODY(6, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(6, 16, 2); else MACM_GRAD_BODY(6, 16, 1);
    }
  } else {
    if (hidden == 32) {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 32, 2); else MACM_GRAD_BODY(4, 32, 1);
    } else {
      if (n_hidden == 2) MACM_GRAD_BODY(4, 16, 2); else MACM_GRAD_BODY(4, 16, 1);
    }
  }
#undef MACM_GRAD_BODY
}

// grad[i] = the sum of partials[q][i] over q in index order: thread (run g, column c) sums the g-th
// quarter of the partials in float64, then run 0's thread adds the four run sums in order and rounds once
__global__ __launch_bounds__(256) void mlp_grad_reduce_kernel(const float* __restrict__ partials, int n_part,
                                                              int n_params, float* __restrict__ grad) {
  __shared__ double run[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  const int per = (n_part + 3) >> 2;
  const int lo = g * per, hi = lo + per < n_part ? lo + per : n_part;
  double s = 0.0;
  if (i < n_params) {
#pragma unroll 8
    for (int q = lo; q < hi; ++q) s = s + (double)partials[(size_t)q * n_params + i];
  }
  run[g][c] = s;
  __syncthreads();
  if (g == 0 && i < n_params) grad[i] = (float)(((run[0][c] + run[1][c]) + run[2][c]) + run[3][c]);
}

long long mlp_grad_partials(long long rows) {
  const long long tiles = (rows + 63) / 64;
  return tiles < kGradMaxPartials ? tiles : kGradMaxPartials;
}

// f(OT{}, n_out as an integral_constant): the instantiation of the gradient kernels for a net and obs type
template <typename F>
static void with_net_instance(const MlpNet& net, bool obs_f64, F&& f) {
  using Pol = std::integral_constant<int, kPolicyLogits>;
  using One = std::integral_constant<int, 1>;
  if (net.n_out == kPolicyLogits) return obs_f64 ? f(double{}, Pol{}) : f(float{}, Pol{});
  return obs_f64 ? f(double{}, One{}) : f(float{}, One{});
}

hipError_t launch_mlp_grad(const MlpNet& net, const void* obs, bool obs_f64, long long rows, const float* dout,
                           float* grad, float* workspace, hipStream_t s) {
  const int n_params = net.n_params();
  if (rows <= 0) return hipMemsetAsync(grad, 0, sizeof(float) * n_params, s);
  const int P = (int)mlp_grad_partials(rows);
  const dim3 grid((unsigned)P), block(64);
  with_net_instance(net, obs_f64, [&](auto ot, auto n_out) {
    hipLaunchKernelGGL((mlp_grad_kernel<decltype(ot), decltype(n_out)::value>), grid, block, 0, s, net.params, net.od,
                       net.hidden, net.n_hidden, (const decltype(ot)*)obs, rows, dout, workspace, n_params);
  });
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((unsigned)((n_params + 63) / 64)), dim3(256), 0, s, workspace, P,
                     n_params, grad);
  return hipGetLastError();
}

// launch_mlp_grad with the loss in the launch; rows > 0 (the caller serves rows = 0)
hipError_t launch_mlp_ppo_grad(const MlpNet& net, const void* obs, bool obs_f64, long long rows, const PpoGradArgs& G,
                               float* grad, float* workspace, hipStream_t s) {
  const int n_params = net.n_params();
  const int P = (int)mlp_grad_partials(rows);
  const dim3 grid((unsigned)P), block(64);
  with_net_instance(net, obs_f64, [&](auto ot, auto n_out) {
    hipLaunchKernelGGL((mlp_ppo_grad_kernel<decltype(ot), decltype(n_out)::value>), grid, block, 0, s, net.params, net.od,
                       net.hidden, net.n_hidden, (const decltype(ot)*)obs, rows, G, workspace, n_params);
  });
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((unsigned)((n_params + 63) / 64)), dim3(256), 0, s, workspace, P,
                     n_params, grad);
  return hipGetLastError();
}

// launch_mlp_ppo_grad through an index and with the advantage's normalisation: the same grid and reduction
hipError_t launch_mlp_ppo_grad_rows(const MlpNet& net, const void* obs, bool obs_f64, long long rows,
                                    const PpoGradArgs& G, const PpoRowsArgs& R, float* grad, float* workspace,
                                    hipStream_t s) {
  const int n_params = net.n_params();
  const int P = (int)mlp_grad_partials(rows);
  const dim3 grid((unsigned)P), block(64);
  with_net_instance(net, obs_f64, [&](auto ot, auto n_out) {
    hipLaunchKernelGGL((mlp_ppo_grad_rows_kernel<decltype(ot), decltype(n_out)::value>), grid, block, 0, s, net.params,
                       net.od, net.hidden, net.n_hidden, (const decltype(ot)*)obs, rows, G, R, workspace, n_params);
  });
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((unsigned)((n_params + 63) / 64)), dim3(256), 0, s, workspace, P,
                     n_params, grad);
  return hipGetLastError();
}

}  // namespace macm
