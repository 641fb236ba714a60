// ppo_row.hpp — one row of the clipped PPO loss (include/macm.h, macm_ppo_loss): from the row's 9 logits
// (its value) to dL/dlogits (dL/dvalue) and the row's terms of the statistics, shared by the one-shot kernels
// (ppo_loss.hip: macm_policy_logp, macm_ppo_loss) and by the loss-to-gradient launches (policy_grad.hip:
// macm_ppo_grad), where it stands between the forward's last layer and the outer products. Both callers
// inline the same functions on the same float32 logits, which is why the fused gradient has the bits of
// logits -> macm_ppo_loss -> macm_policy_grad.
//
// All arithmetic is float64 on the float32 inputs, every operation rounded once (-ffp-contract=off,
// hipflags.mk), in the association written here; what is stored as float32 is one rounding of a float64.
// exp and log are the device library's float64 functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_mlp.hpp"

namespace macm {

// macm_ppo_config without its reserved words
struct PpoCfg {
  float clip, vf_coef, ent_coef, vf_clip;
};

// A stat partial: the sums over some rows of the row terms below (ratio: the maximum), 8 doubles
constexpr int kPpoStatSlots = 8;
enum { kPpoPl = 0, kPpoH = 1, kPpoKl = 2, kPpoClipped = 3, kPpoRatioMax = 4, kPpoVl = 5 };
constexpr int kPpoPolicyTerms = 5;  // slots 0..4 are the policy half's, slot 5 the value half's

struct PpoPolicyTerms {
  double pl, H, kl, clipped, ratio;
};

// Per head h: p[3h + c] the softmax, lp[3h + c] the log-softmax, Hh[h] the entropy; returns the
// log-probability of the taken actions (an action byte above 2 counts as 2)
__device__ __forceinline__ double ppo_logp_row(const float (&z)[9], const uint8_t (&a)[3], double (&p)[9],
                                               double (&lp)[9], double (&Hh)[3]) {
  double taken[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const double z0 = (double)z[3 * h], z1 = (double)z[3 * h + 1], z2 = (double)z[3 * h + 2];
    double m = z0 > z1 ? z0 : z1;
    m = m > z2 ? m : z2;
    const double e0 = exp(z0 - m), e1 = exp(z1 - m), e2 = exp(z2 - m);
    const double S = (e0 + e1) + e2;
    const double lse = m + log(S);
    lp[3 * h] = z0 - lse;
    lp[3 * h + 1] = z1 - lse;
    lp[3 * h + 2] = z2 - lse;
    p[3 * h] = e0 / S;
    p[3 * h + 1] = e1 / S;
    p[3 * h + 2] = e2 / S;
    Hh[h] = -((p[3 * h] * lp[3 * h] + p[3 * h + 1] * lp[3 * h + 1]) + p[3 * h + 2] * lp[3 * h + 2]);
    taken[h] = a[h] == 0 ? lp[3 * h] : a[h] == 1 ? lp[3 * h + 1] : lp[3 * h + 2];
  }
  return (taken[0] + taken[1]) + taken[2];
}

// The policy half of row r: d[3h + c] = k (g_logp (1[c = a_h] - p_hc) + c_e p_hc (lp_hc + H_h)) with
// k = scale / rows, and the row's terms. logp is rounded to float32 before old_logp is subtracted, so an
// old_logp that macm_policy_logp stored from the same logits gives ratio = 1 exactly.
__device__ __forceinline__ void ppo_policy_row(const float (&z)[9], const uint8_t (&a)[3], float old_logp, float adv,
                                               const PpoCfg& cfg, double k, float (&d)[9], PpoPolicyTerms& T) {
  double p[9], lp[9], Hh[3];
  const float logp32 = (float)ppo_logp_row(z, a, p, lp, Hh);
  const double ratio = exp((double)logp32 - (double)old_logp);
  const double eps = (double)cfg.clip, A = (double)adv;
  const double lo = 1.0 - eps, hi = 1.0 + eps;
  double rc = ratio > lo ? ratio : lo;  // clamp(ratio, lo, hi) = min(max(ratio, lo), hi)
  rc = rc < hi ? rc : hi;
  const double s1 = ratio * A, s2 = rc * A;
  const bool unclipped = s1 <= s2;  // a tie takes the unclipped branch
  const double g = unclipped ? -A * ratio : 0.0;
  const double ce = (double)cfg.ent_coef;
  T.pl = -(unclipped ? s1 : s2);
  T.H = (Hh[0] + Hh[1]) + Hh[2];
  T.kl = (ratio - 1.0) - log(ratio);
  T.clipped = fabs(ratio - 1.0) > eps ? 1.0 : 0.0;
  T.ratio = ratio;
#pragma unroll
  for (int h = 0; h < 3; ++h) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int q = 3 * h + c;
      const double ind = a[h] == c || (c == 2 && a[h] > 2) ? 1.0 : 0.0;
      d[q] = (float)(k * (g * (ind - p[q]) + ce * (p[q] * (lp[q] + Hh[h]))));
    }
  }
}

// The value half of row r: returns k c_v g_v as float32, vl the row's value loss. Without old values
// vl = (v - ret)^2 / 2; with them the larger of that and the same of the clipped value
// vc = old_v + clamp(v - old_v, -vf_clip, vf_clip), whose gradient is zero where the clamp is active.
__device__ __forceinline__ float ppo_value_row(float v, float ret, bool has_old, float old_v, const PpoCfg& cfg,
                                               double k, double& vl) {
  const double dv = (double)v - (double)ret;
  const double u = dv * dv;
  double g = dv;
  vl = 0.5 * u;
  if (has_old) {
    const double ev = (double)cfg.vf_clip, diff = (double)v - (double)old_v;
    double cl = diff > -ev ? diff : -ev;
    cl = cl < ev ? cl : ev;
    const double dc = ((double)old_v + cl) - (double)ret;
    const double c = dc * dc;
    if (!(u >= c)) {
      vl = 0.5 * c;
      g = fabs(diff) <= ev ? dc : 0.0;
    }
  }
  return (float)(k * ((double)cfg.vf_coef * g));
}

// host side (C++ linkage, capi_learn.hip). ppo_loss.hip: the one-shot kernels and the reduction of the stat
// partials; policy_grad.hip: the loss-to-gradient launch of one net.
constexpr int kPpoBlock = 256;         // ppo_loss_kernel: threads per block, one row per thread and stride
constexpr int kPpoMaxBlocks = 2048;    // ... and at most this many blocks, one stat partial each
long long ppo_loss_partials(long long rows);  // min(ceil(rows / kPpoBlock), kPpoMaxBlocks)

struct PpoLossArgs {
  const float* logits;      // [rows, 9] or NULL
  const uint8_t* actions;   // [rows, 3]
  const float* old_logp;    // [rows]
  const float* adv;         // [rows]
  const float* values;      // [rows] or NULL
  const float* ret;         // [rows]
  const float* old_values;  // [rows] or NULL
  const float* scale;       // one float or NULL
  float* dlogits;           // [rows, 9] or NULL
  float* dvalues;           // [rows] or NULL
  double* part;             // [ppo_loss_partials(rows)][kPpoStatSlots] or NULL
  PpoCfg cfg;
};
hipError_t launch_policy_logp(const float* logits, const uint8_t* actions, long long rows, float* logp,
                              float* entropy, hipStream_t s);
hipError_t launch_ppo_loss(const PpoLossArgs& A, long long rows, hipStream_t s);
// stats[8] from n_part partials; a half that was not computed counts as 0 and its slots are not read
hipError_t launch_ppo_stats(const double* part, int n_part, long long rows, const PpoCfg& cfg, bool has_policy,
                            bool has_value, double* stats, hipStream_t s);

// What the loss-to-gradient launch takes in the place of dout
struct PpoGradArgs {
  const uint8_t* actions;   // the policy: [rows, 3]
  const float* old_logp;    // the policy: [rows]
  const float* adv;         // the policy: [rows]
  const float* ret;         // the critic: [rows]
  const float* old_values;  // the critic: [rows] or NULL
  PpoCfg cfg;
  double k;                 // 1 / rows
  double* stat;             // [mlp_grad_partials(rows)][kPpoStatSlots], or NULL: no stats wanted, none summed
};
hipError_t launch_mlp_ppo_grad(const MlpNet& net, const void* obs, bool obs_f64, long long rows, const PpoGradArgs& G,
                               float* grad, float* workspace, hipStream_t s);

// What macm_ppo_grad_rows adds to that: position r of the call reads source row index[r] of obs and of G's
// arrays, and the row's advantage is normalised as it is loaded. A position whose source row is outside
// [0, n_src) is a tail lane: nothing of it is loaded.
struct PpoRowsArgs {
  const int32_t* index;  // [rows], or NULL: positions are rows (n_src is not read)
  long long n_src;       // the source arrays' rows, at most 2^31 - 1
  const double* norm;    // {mean, rstd}: adv = (float)(((double)adv - mean) rstd), or NULL
};
hipError_t launch_mlp_ppo_grad_rows(const MlpNet& net, const void* obs, bool obs_f64, long long rows,
                                    const PpoGradArgs& G, const PpoRowsArgs& R, float* grad, float* workspace,
                                    hipStream_t s);

// macm_adv_moments (ppo_loss.hip): out = {mean, rstd, std, n} of x[index[r]] (index NULL: x[r]) over the
// positions whose source row is in [0, n_src); part holds 2 doubles per block, ppo_loss_partials(rows) blocks
hipError_t launch_adv_moments(const float* x, const int32_t* index, long long n_src, long long rows, double eps,
                              double* out, double* part, hipStream_t s);

// macm_ppo_adam (ppo_adam.hip): one workgroup of kAdamBlock threads steps both nets, [0] the policy and [1]
// the critic; a net that is absent has n = 0 and its pointers are never followed. head is the state's
// double[8] (include/macm.h), m and v the state's float32 moments
constexpr int kAdamBlock = 256;
constexpr int kAdamHead = 8;
struct AdamArgs {
  float* param[2];
  const float* grad[2];
  float* m[2];
  float* v[2];
  int n[2];
  double* head;
  const double* stats;  // [8] or NULL: stats[4] is approx_kl
  double lr, beta1, beta2, omb1, omb2, eps;  // omb: 1 - beta, formed on the host
  double max_grad_norm, target_kl;
};
hipError_t launch_ppo_adam(const AdamArgs& A, hipStream_t s);

}  // namespace macm
