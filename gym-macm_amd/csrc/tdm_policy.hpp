// tdm_policy.hpp — one TDM agent's decision of a learned set policy: a permutation-invariant float32 net
// over the agent's [N-1, 4] observation slots, shared by the one-shot kernel (tdm_policy.hip,
// macm_policy_tdm) and the closed-loop TDM rollouts (flock_step_w64.hip / rollout_autoreset.inc,
// macm_tdm_rollout_policy), where it stands in the place of the scripted bot (bots.hpp, bot_combat_row).
//
// The definition (include/macm.h, macm_tdm_policy), all float32, the conventions of policy_mlp.hpp:
//   encoder: for every slot k with m[k] != 0: e_k[j] = relu(b1[j] + sum_q W1[q][j] (float)o[k][q]), q ascending
//   pool   : g[j] = +0, then g[j] = e_k[j] > g[j] ? e_k[j] : g[j] over the live slots (after the relu no e is
//            NaN or negative, so the order of the slots does not matter)
//   trunk  : u = (g[0..H-1], health); t[j] = relu(b2[j] + sum_k W2[k][j] u[k]), k = 0..H ascending
//   head   : z[c] = b3[c] + sum_k W3[k][c] t[k]; 11 logits of MultiDiscrete([3, 3, 3, 2]): head h < 3 at
//            z[3h + c], head 3 at z[9], z[10]
//   action : per head the lowest c with the largest z (+ noise, one float32 add), by `>` from -inf
// lane = agent: every weight is a wave-uniform operand read through the constant address space (scalar
// loads), no LDS. The slot loop is not divergent: a masked slot's encoder output is computed and dropped
// by the select that pools (its relu output is a number whatever the slot holds). Two loop orders of the
// encoder give the same bits (tdm_policy_row_t): in chunks of kTdmEncChunk outputs, each over all the slots
// with its weights held in SGPRs (live set: the pool, H VGPRs, and a few slots' inputs), or slot by slot
// over all H outputs (the pool and one slot's e: 2 H VGPRs).
#pragma once
#include "flock_common.hpp"
#include "policy_mlp.hpp"

namespace macm {

constexpr int kTdmPolicyLogits = 11;  // MultiDiscrete([3, 3, 3, 2]): heads 0..2 at [3h + c], head 3 at [9], [10]
constexpr int kTdmEncChunk = 8;       // encoder outputs per pass over the slots (divides H = 16 and 32)

// floats of the params: W1[4][H], b1[H], W2[H + 1][H], b2[H], W3[H][11], b3[11]
constexpr int tdm_policy_n_params(int H) { return 4 * H + H + (H + 1) * H + H + H * kTdmPolicyLogits + kTdmPolicyLogits; }

// What the kernels take of a registered TDM policy and of one call (device pointers)
struct TdmPolicyArgs {
  const float* params;  // 16-byte aligned
  const float* noise;   // [rows, 11] or NULL
  float* logits;        // [rows, 11] or NULL
  int32_t hidden;       // H: 16 or 32
  uint32_t team_mask;   // rollouts: bit t set = team t takes the policy, the other teams bots.combat
};

template <typename OT>
__device__ __forceinline__ void tdm_slot_load(const OT* __restrict__ o, float (&x)[4]) {
  if constexpr (sizeof(OT) == 4) {
    const float4 v = *reinterpret_cast<const float4*>(o);  // a slot is 16 bytes, 16-byte aligned
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    const double2 a = *reinterpret_cast<const double2*>(o), b = *reinterpret_cast<const double2*>(o + 2);
    x[0] = (float)a.x, x[1] = (float)a.y, x[2] = (float)b.x, x[3] = (float)b.y;
  }
}

template <typename OT, int H, bool CHUNKED>
__device__ __forceinline__ void tdm_policy_row_t(policy_cptr p, const OT* __restrict__ o, const uint8_t* __restrict__ m,
                                                 int S, float health, const float* __restrict__ noise,
                                                 uint8_t* __restrict__ act, float* __restrict__ logits) {
  float u[H + 1];
  if constexpr (CHUNKED) {
    // The encoder and the pool, kTdmEncChunk outputs at a time over all the slots: the chunk's 5 x 8 weights
    // are fetched once and stay in SGPRs across the slot loop, and the slots are read once per chunk. The
    // form of the rollout launches, where a wave has few others beside it to cover a scalar load's latency
    // (measured there: 236 -> 135 us per step at 4096 envs of 2 x 16). Every e_k[j] is the same
    // chain and the pool visits the slots in the same order, so the bits are those of the other form.
#pragma unroll
    for (int c = 0; c < H / kTdmEncChunk; ++c) {
      float w[4][kTdmEncChunk], b[kTdmEncChunk], g[kTdmEncChunk];
#pragma unroll
      for (int j = 0; j < kTdmEncChunk; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q][j] = p[q * H + c * kTdmEncChunk + j];
        b[j] = p[4 * H + c * kTdmEncChunk + j];
        g[j] = 0.0f;
      }
#pragma unroll 4
      for (int k = 0; k < S; ++k) {
        float x[4];
        tdm_slot_load<OT>(o + (size_t)k * 4, x);
        const bool live = m[k] != 0;
#pragma unroll
        for (int j = 0; j < kTdmEncChunk; ++j) {
          float e = b[j];
#pragma unroll
          for (int q = 0; q < 4; ++q) e = __builtin_fmaf(w[q][j], x[q], e);
          e = e > 0.0f ? e : 0.0f;
          g[j] = live && e > g[j] ? e : g[j];
        }
      }
#pragma unroll
      for (int j = 0; j < kTdmEncChunk; ++j) u[c * kTdmEncChunk + j] = g[j];
    }
  } else {
    // Slot by slot over all H outputs: every slot is read once (the one-shot kernel's rows come from HBM,
    // lane-strided) and the 5 H weights are fetched again for every slot, which a full device of 256-row
    // blocks covers (measured there: 89 us per step of the per-step loop against 146 with the chunks).
#pragma unroll
    for (int j = 0; j < H; ++j) u[j] = 0.0f;
#pragma nounroll
    for (int k = 0; k < S; ++k) {
      float x[4], e[H];
      tdm_slot_load<OT>(o + (size_t)k * 4, x);
      const bool live = m[k] != 0;
      policy_layer<4, H, true>(p, p + 4 * H, x, e);
#pragma unroll
      for (int j = 0; j < H; ++j) u[j] = live && e[j] > u[j] ? e[j] : u[j];
    }
  }
  u[H] = health;
  p += 4 * H + H;
  float t[H];
  policy_layer<H + 1, H, true>(p, p + (H + 1) * H, u, t);
  p += (H + 1) * H + H;
  float z[kTdmPolicyLogits];
  policy_layer<H, kTdmPolicyLogits, false>(p, p + H * kTdmPolicyLogits, t, z);
  if (logits) {
#pragma unroll
    for (int j = 0; j < kTdmPolicyLogits; ++j) logits[j] = z[j];
  }
  if (noise) {
#pragma unroll
    for (int j = 0; j < kTdmPolicyLogits; ++j) z[j] = z[j] + noise[j];
  }
  uint8_t a[4];
#pragma unroll
  for (int hd = 0; hd < 4; ++hd) {
    int best = 0;
    float bz = -__builtin_inff();
#pragma unroll
    for (int c = 0; c < (hd < 3 ? 3 : 2); ++c) {
      if (z[3 * hd + c] > bz) {
        best = c;
        bz = z[3 * hd + c];
      }
    }
    a[hd] = (uint8_t)best;
  }
  *reinterpret_cast<uchar4*>(act) = make_uchar4(a[0], a[1], a[2], a[3]);
}

// o: the agent's [N-1, 4] obs slots as stored, m: their mask, health: the agent's health rounded to
// float32; noise / logits: its 11 floats or NULL; act: its 4 action bytes (4-aligned). M.params and
// M.hidden must be wave-uniform. CHUNKED: the encoder's loop order (the same bits either way): the rollout
// launches take the chunks, the one-shot kernel the slots.
template <typename OT, bool CHUNKED>
__device__ __forceinline__ void tdm_policy_row(const TdmPolicyArgs& M, const OT* __restrict__ o,
                                               const uint8_t* __restrict__ m, int N, float health,
                                               const float* __restrict__ noise, uint8_t* __restrict__ act,
                                               float* __restrict__ logits) {
  const policy_cptr p = (policy_cptr)(unsigned long long)M.params;
  if (M.hidden == 32)
    tdm_policy_row_t<OT, 32, CHUNKED>(p, o, m, N - 1, health, noise, act, logits);
  else
    tdm_policy_row_t<OT, 16, CHUNKED>(p, o, m, N - 1, health, noise, act, logits);
}

// host side (tdm_policy.hip): the decision over `rows` agent rows. agents [N] or NULL: rows whose
// agents[row % N] is 0 are left untouched. reset [rows / N] or NULL with init_health: the agents of an
// env whose flag is set read init_health (the per-step loop of an autoreset world: the step's health
// output keeps the terminal health of a reset env).
hipError_t launch_policy_tdm(const TdmPolicyArgs& M, const void* obs, const uint8_t* mask, const double* health,
                             bool obs_f64, int N, long long rows, const uint8_t* agents, const uint8_t* reset,
                             double init_health, uint8_t* act, hipStream_t s);

// host side (tdm_policy_grad.hip): dL/dparams of the set policy from dlogits [rows, 11] (macm_tdm_policy_grad);
// M.noise, M.logits and M.team_mask are not read. One wave writes one partial [tdm_policy_n_params(hidden)]
// into the workspace, mlp_grad_partials(rows) of them (policy_mlp.hpp); rows <= 0 writes zeros.
hipError_t launch_tdm_policy_grad(const TdmPolicyArgs& M, const void* obs, const uint8_t* mask, const double* health,
                                  bool obs_f64, int N, long long rows, const uint8_t* agents, const float* dlogits,
                                  float* grad, float* workspace, hipStream_t s);

}  // namespace macm
