// tdm_policy_grad.hip — parameter gradients of the TDM set policy (macm_tdm_policy_grad): from dL/dlogits of
// every agent row to dL/dparams, one launch plus a small reduction, in the shape of policy_grad.hip.
//
// The definition (include/macm.h): the forward is tdm_policy.hpp's, bit for bit; with e_k the encoder output
// of live slot k, g the pool, u = (g, health), t the trunk's stored activation and d3 the row's dlogits
//   gW3[k][c] = sum_r t[r][k] d3[r][c]                 gb3[c] = sum_r d3[r][c]
//   d2[r][j]  = t[r][j] > 0 ? sum_c W3[j][c] d3[r][c] : 0
//   gW2[k][j] = sum_r u[r][k] d2[r][j], k = 0..H       gb2[j] = sum_r d2[r][j]
//   dg[r][j]  = g[r][j] > 0 ? sum_i W2[j][i] d2[r][i] : 0
//   gW1[q][j] = sum_r o[r][k*][q] dg[r][j]             gb1[j] = sum_r dg[r][j]
// where k*(r, j) is the lowest live slot with e_k[j] == g[j], and only where g[j] > 0: the slot at which the
// forward's `e > g ? e : g` scan last changed g[j]. All float32; no atomics, every sum's association fixed by
// `rows` alone.
//
// Per-row part (VALU): one wave per block, lane = row, tiles of 64 rows. The forward is tdm_policy_row_t's slot
// by slot form (policy_layer over a slot, then the strict-> select) with arg[j], the slot of the select's last
// update, tracked beside g[j]: 2 H registers across the slot loop and H for the slot's e. A lane without a
// row (past `rows`, or an agent the call skips) loads nothing: its slots read as zeros under a dead mask, its
// health and dlogits as zeros, so g = 0, every d of it is an exact zero and so is each of its products. d2 and
// dg are grad_back_layer's j-ordered fmaf chains over wave-uniform weights (dg over the first H rows of W2:
// the health row has no gradient to pass on).
//
// Layers 2 and 3 (MFMA): gW3 = T^T D3 and gW2[0..H-1] = G^T D2 through grad_outer, as policy_grad.hip's. u has
// H + 1 entries, one more than a block at H = 32, so the health row and gb2 ride together in a third product
// with A = (health, 1): rows 0 and 1 of its block are W2's row H and b2, which are adjacent in params. gb3 is
// a lane-local sum over the wave's tiles, reduced through LDS in lane order at the end.
//
// Layer 1 is not an outer product: the A operand (the winning slot) differs per unit. Eight units at a time,
// each lane gathers the winner's four inputs (one 16-byte load at o + 4 arg[j], only where g[j] > 0) and writes
// the five terms o[k*][q] dg[j] (q = 0..3) and dg[j] into five LDS images [64 rows][9]; lane l < 40 then adds
// column l (term l >> 3 of unit 8 c + (l & 7)) over the 64 rows in row order onto a lane-local accumulator
// that lives across the wave's tiles: H / 8 accumulators per lane, no cross-lane step at the end. The images
// are 584 floats apart (64 * 9 + 8): the writes have stride 9 across lanes and the 40 readers fall into 40
// banks. They lie over the outer products' operand images, between the same barriers.
//
// Cross-wave reduction: as policy_grad.hip's. P = min(tiles, kGradMaxPartials) waves; wave w takes tiles w,
// w + P, ... (64-bit row indices) and writes one partial [n_params]; tdm_grad_reduce_kernel sums the partials
// per parameter in index order in float64 (four contiguous runs, then the run sums in order), rounds once.
#include <type_traits>

#include "policy_grad.hpp"
#include "tdm_policy.hpp"

namespace macm {

constexpr int kTdmGradChunk = 8;                       // units per pass of layer 1
constexpr int kTdmGradTermLds = kTdmGradChunk + 1;     // floats per row of a term image
constexpr int kTdmGradTermImage = 64 * kTdmGradTermLds + 8;  // floats from one term's image to the next
static_assert(5 * kTdmGradTermImage <= 2 * 64 * kGradLds, "the term images lie over the operand images");

// The encoder and the pool of tdm_policy_row_t (slot by slot), with arg[j]: the slot of g[j]'s last update
template <typename OT, int H>
__device__ __forceinline__ void tdm_grad_pool(policy_cptr p, const OT* __restrict__ o, const uint8_t* __restrict__ m,
                                              int S, bool has_row, float (&g)[H], int (&arg)[H]) {
#pragma unroll
  for (int j = 0; j < H; ++j) {
    g[j] = 0.0f;
    arg[j] = 0;
  }
#pragma nounroll
  for (int k = 0; k < S; ++k) {
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, e[H];
    bool live = false;
    if (has_row) {
      tdm_slot_load<OT>(o + (size_t)k * 4, x);
      live = m[k] != 0;
    }
    policy_layer<4, H, true>(p, p + 4 * H, x, e);
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const bool up = live && e[j] > g[j];
      g[j] = up ? e[j] : g[j];
      arg[j] = up ? k : arg[j];
    }
  }
}

template <typename OT, int H>
__global__ __launch_bounds__(64) void tdm_policy_grad_kernel(const float* __restrict__ params,
                                                             const OT* __restrict__ obs,
                                                             const uint8_t* __restrict__ mask,
                                                             const double* __restrict__ health, int N, long long rows,
                                                             const uint8_t* __restrict__ agents,
                                                             const float* __restrict__ dlogits,
                                                             float* __restrict__ partials) {
  constexpr int NP = tdm_policy_n_params(H), NC = H / kTdmGradChunk;
  __shared__ __attribute__((aligned(16))) float sm[2 * 64 * kGradLds];
  float* const sA = sm;
  float* const sB = sm + 64 * kGradLds;
  const int lane = threadIdx.x, S = N - 1;
  const long long tiles = (rows + 63) >> 6;
  const policy_cptr W1 = (policy_cptr)(unsigned long long)params;
  const policy_cptr W2 = W1 + 4 * H + H, b2 = W2 + (H + 1) * H;
  const policy_cptr W3 = b2 + H;
  float* const part = partials + (size_t)blockIdx.x * NP;

  grad_f32x16 acc2, acch, acc3;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc2[q] = acch[q] = acc3[q] = 0.0f;
  float bs3[kTdmPolicyLogits], acc1[NC];
#pragma unroll
  for (int j = 0; j < kTdmPolicyLogits; ++j) bs3[j] = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc1[c] = 0.0f;

  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long r = t * 64 + lane;
    const bool has_row = r < rows && (!agents || agents[r % N] != 0);
    const OT* const o = obs + r * S * 4;  // (followed only where has_row)
    float g[H], d3[kTdmPolicyLogits], hx[2] = {0.0f, 1.0f};
    int arg[H];
    tdm_grad_pool<OT, H>(W1, o, mask + r * S, S, has_row, g, arg);
#pragma unroll
    for (int j = 0; j < kTdmPolicyLogits; ++j) d3[j] = 0.0f;
    if (has_row) {
      hx[0] = (float)health[r];
#pragma unroll
      for (int j = 0; j < kTdmPolicyLogits; ++j) d3[j] = dlogits[r * kTdmPolicyLogits + j];
    }
    float d2[H], dg[H];
    {
      float u[H + 1], tt[H];
#pragma unroll
      for (int j = 0; j < H; ++j) u[j] = g[j];
      u[H] = hx[0];
      policy_layer<H + 1, H, true>(W2, b2, u, tt);
      grad_outer<H, kTdmPolicyLogits>(sA, sB, tt, d3, acc3, lane);
      grad_back_layer<H, kTdmPolicyLogits>(W3, tt, d3, d2);
    }
#pragma unroll
    for (int j = 0; j < kTdmPolicyLogits; ++j) bs3[j] = bs3[j] + d3[j];
    grad_outer<H, H>(sA, sB, g, d2, acc2, lane);
    grad_outer<2, H>(sA, sB, hx, d2, acch, lane);  // W2's health row and b2
    grad_back_layer<H, H>(W2, g, d2, dg);

    // layer 1, kTdmGradChunk units at a time: the winners' terms into the images, their column sums onto acc1
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      __syncthreads();  // the reads of the images' last use are done
#pragma unroll
      for (int jj = 0; jj < kTdmGradChunk; ++jj) {
        const int j = c * kTdmGradChunk + jj;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g[j] > 0.0f) tdm_slot_load<OT>(o + (size_t)arg[j] * 4, x);  // g > 0: a lane with a row, a live slot
        float* const im = sm + lane * kTdmGradTermLds + jj;
#pragma unroll
        for (int q = 0; q < 4; ++q) im[q * kTdmGradTermImage] = x[q] * dg[j];
        im[4 * kTdmGradTermImage] = dg[j];
      }
      __syncthreads();
      if (lane < 5 * kTdmGradChunk) {
        const float* const col = sm + (lane >> 3) * kTdmGradTermImage + (lane & 7);
        float s = acc1[c];
        for (int rr = 0; rr < 64; ++rr) s = s + col[rr * kTdmGradTermLds];
        acc1[c] = s;
      }
    }
  }

  // the wave's partial, in the layout of params: W1[4][H], b1[H], W2[H + 1][H], b2[H], W3[H][11], b3[11]
  if (lane < 5 * kTdmGradChunk) {
#pragma unroll
    for (int c = 0; c < NC; ++c) part[(lane >> 3) * H + c * kTdmGradChunk + (lane & 7)] = acc1[c];
  }
  float* o2 = part + 4 * H + H;
  grad_store_block<H, H>(acc2, o2, lane);
  grad_store_block<2, H>(acch, o2 + H * H, lane);
  float* o3 = o2 + (H + 1) * H + H;
  grad_store_block<H, kTdmPolicyLogits>(acc3, o3, lane);
  grad_store_bias<kTdmPolicyLogits>(sB, bs3, o3 + H * kTdmPolicyLogits, lane);
}

// grad[i] = the sum of partials[q][i] over q in index order, the definition of policy_grad.hip's
// mlp_grad_reduce_kernel: thread (run g, column c) sums the g-th quarter of the partials in float64, then run
// 0's thread adds the four run sums in order and rounds once
__global__ __launch_bounds__(256) void tdm_grad_reduce_kernel(const float* __restrict__ partials, int n_part,
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

hipError_t launch_tdm_policy_grad(const TdmPolicyArgs& M, const void* obs, const uint8_t* mask, const double* health,
                                  bool obs_f64, int N, long long rows, const uint8_t* agents, const float* dlogits,
                                  float* grad, float* workspace, hipStream_t s) {
  const int n_params = tdm_policy_n_params(M.hidden);
  if (rows <= 0) return hipMemsetAsync(grad, 0, sizeof(float) * n_params, s);
  const int P = (int)mlp_grad_partials(rows);
  const dim3 grid((unsigned)P), block(64);
  auto launch = [&](auto ot, auto h) {
    using OT = decltype(ot);
    hipLaunchKernelGGL((tdm_policy_grad_kernel<OT, decltype(h)::value>), grid, block, 0, s, M.params, (const OT*)obs,
                       mask, health, N, rows, agents, dlogits, workspace);
  };
  using H16 = std::integral_constant<int, 16>;
  using H32 = std::integral_constant<int, 32>;
  if (M.hidden == 32) {
    if (obs_f64) launch(double{}, H32{}); else launch(float{}, H32{});
  } else {
    if (obs_f64) launch(double{}, H16{}); else launch(float{}, H16{});
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(tdm_grad_reduce_kernel, dim3((unsigned)((n_params + 63) / 64)), dim3(256), 0, s, workspace, P,
                     n_params, grad);
  return hipGetLastError();
}

}  // namespace macm
