// launch.hpp — the host side of the env kernels: every function one translation unit defines and another
// calls, declared once (default arguments here only), and the bundles of what travels together down the
// call chain C-ABI entry point -> launcher -> kernel. Every unit that defines one of these includes this
// header, so a definition that drifts from its declaration is an ambiguous call, not a new overload.
// The bundles are host structs: never a kernel parameter (the kernels' argument structs are
// flock_common.hpp's and flock_step_w64.hip's). The launchers of the learned-policy kernels are declared
// in policy_mlp.hpp, tdm_policy.hpp and ppo_row.hpp.
#pragma once
#include "flock_common.hpp"
#include "policy_mlp.hpp"
#include "tdm_policy.hpp"

namespace macm {

// One step's inputs and outputs (device pointers; an output that is NULL is not written): what Flock and
// TDM launches share, ...
struct StepIO {
  const void* actions = nullptr;
  void* obs = nullptr;
  bool obs_f64 = false;  // the type behind obs
  uint8_t* done = nullptr;
};
// ... a Flock launch's, ...
struct FlockIO : StepIO {
  int32_t* nbr = nullptr;
  float* rew = nullptr;
  uint8_t* coll = nullptr;
};
// ... and a TDM launch's (its other outputs: TdmBuffers' *_out)
struct TdmIO : StepIO {
  int32_t* hit_out = nullptr;  // non-NULL: the kernels that record the combat events (macm_tdm_set_events)
  // closed-loop rollouts: the set policy of the policy's teams where the bot is (NULL: the bot everywhere)
  const TdmPolicyArgs* policy = nullptr;
};

// A rollout launch: nsteps steps, step k's actions at actions + k * astride bytes (0: the closed loop,
// actions is the actor's buffer), traj: step k's outputs in row k of [K, ...] buffers
struct RollShape {
  int nsteps = 0;
  unsigned long long astride = 0;
  int traj = 0;
  RollShape(int nsteps_, unsigned long long astride_, bool traj_) : nsteps(nsteps_), astride(astride_), traj(traj_) {}
};

// The tail observation of a TDM trajectory rollout (flock_step_w64.hip TailObs); default-constructed: off
struct TailLaunch {
  unsigned long long* ctl = nullptr;  // tail_ctl_words(E) counters and ready words
  unsigned tag = 0u;                  // this launch's tag (0: off)
  int workers = 0;                    // observe-only blocks beyond the envs
  int k0 = 0;                         // the first step observed in the tail
};

// What the in-launch episode reset needs (worlds with autoreset on)
struct ResetLaunch {
  uint32_t* mt;  // [E][kMtStride] the envs' streams
  PoseDraw D;
  FinalOut F;
  ResetLaunch(uint32_t* mt_, const PoseDraw& D_, const FinalOut& F_) : mt(mt_), D(D_), F(F_) {}
};

// A Flock rollout's extras: debug bit 0 MACM_DEBUG_ROLLOUT_RELOAD (load and fence every step), bit 1
// MACM_DEBUG_NEAR_PLAIN; the closed loop's MLP policy where the bot is (NULL: the bot), the critic
// beside it (NULL: none) and the policy's own draw (worlds with sampling on; NULL: it reads policy->noise)
struct FlockRollExtras {
  int debug = 0;
  const PolicyArgs* policy = nullptr;
  const ValueArgs* critic = nullptr;
  const SampleArgs* sample = nullptr;
  const TdmPolicyArgs* tdm_policy = nullptr;  // TDM rollouts: TdmIO::policy
};

// launch_final_copy's sources: the step's output rows ([E, ...]) and their sizes per env
struct FinalRows {
  const void* obs = nullptr;
  const int32_t* nbr = nullptr;
  const uint8_t* msk = nullptr;
  unsigned long long obs_bytes = 0;
  int n_nbr = 0, n_msk = 0;
};

// f(OT{}) with the type behind an obs pointer
template <typename F>
void with_obs_type(bool obs_f64, F&& f) {
  if (obs_f64) f(double{});
  else f(float{});
}

// ---- flock_step_w64.hip: the wave kernels (N <= 64), one-step, reset and observe
hipError_t launch_step_w64(const StepParams& P, const WorldBuffers& B, int cur, const FlockIO& io, hipStream_t s);
hipError_t launch_init_w64(const StepParams& P, const WorldBuffers& B, int cur, void* obs, bool obs_f64,
                           int32_t* nbr, const uint8_t* mask, hipStream_t s);
hipError_t launch_observe_w64(const StepParams& P, const WorldBuffers& B, void* obs, bool obs_f64, int32_t* nbr,
                              hipStream_t s);
hipError_t launch_tdm_step_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                               const TdmBuffers& TB, int cur, const TdmIO& io, hipStream_t s);
hipError_t launch_tdm_init_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                               const TdmBuffers& TB, int cur, void* obs, bool obs_f64, const uint8_t* mask,
                               hipStream_t s);
hipError_t launch_tdm_observe_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                  const TdmBuffers& TB, void* obs, bool obs_f64, hipStream_t s);
// ---- flock_rollout_w64.hip: the rollouts of the wave kernels
hipError_t launch_rollout_w64(const StepParams& P, const WorldBuffers& B, int cur, const FlockIO& io,
                              const RollShape& sh, const FlockRollExtras& x, hipStream_t s);
hipError_t launch_tdm_rollout_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                  const TdmBuffers& TB, int cur, const TdmIO& io, const RollShape& sh,
                                  const TailLaunch& tail, hipStream_t s);
int tdm_rollout_resident_blocks(int n_agents, bool obs_f64);
// order[0..E): the envs by descending contact-list size; reset2: Handoff::ctr, zeroed for the step (or NULL)
hipError_t launch_env_order(const uint32_t* ccount, uint32_t* order, int E, int C, hipStream_t s,
                            unsigned int* reset2 = nullptr);
// ---- flock_rollout_ar_w64.hip: the rollouts with the in-launch episode reset (worlds with autoreset on)
hipError_t launch_rollout_ar_w64(const StepParams& P, const WorldBuffers& B, int cur, const FlockIO& io,
                                 const RollShape& sh, const FlockRollExtras& x, const ResetLaunch& r, hipStream_t s);
hipError_t launch_tdm_rollout_ar_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                     const TdmBuffers& TB, int cur, const TdmIO& io, const RollShape& sh,
                                     const ResetLaunch& r, hipStream_t s);
// ---- flock_step_wg.hip: the workgroup kernels (64 < N <= 1024)
int wg_block(int N);
int wg_lds_bytes(int N, int tcap);
hipError_t wg_configure(int N, int tcap);
// HS: the B -> C handoff (NULL: kernel C after B on s); bot_act: kernel C's fused bot writes its actions there
hipError_t launch_step_wg(const StepParams& P, const WorldBuffers& B, int cur, int tcap, const FlockIO& io,
                          hipStream_t s, HandoffStream* HS, uint8_t* bot_act = nullptr);
hipError_t launch_init_wg(const StepParams& P, const WorldBuffers& B, int cur, void* obs, bool obs_f64, int32_t* nbr,
                          const uint8_t* mask, hipStream_t s);
hipError_t launch_observe_wg(const StepParams& P, const WorldBuffers& B, void* obs, bool obs_f64, int32_t* nbr,
                             hipStream_t s);
// ---- flock_big.hip: worlds of 1024 < N <= 4096 agents
hipError_t big_configure(int N);
int big_step_lds(int N);
int big_init_lds(int N);
hipError_t launch_step_big(const StepParams& P, const WorldBuffers& B, int cur, const FlockIO& io, hipStream_t s);
hipError_t launch_init_big(const StepParams& P, const WorldBuffers& B, int cur, void* obs, bool obs_f64, int32_t* nbr,
                           const uint8_t* mask, hipStream_t s);
hipError_t launch_observe_big(const StepParams& P, const WorldBuffers& B, void* obs, bool obs_f64, int32_t* nbr,
                              hipStream_t s);
// ---- tdm_step_wg.hip: the TDM workgroup step (N > 64)
hipError_t tdm_wg_configure(int N);
int tdm_wg_step_lds(int N);
int tdm_wg_obs_lds(int N);
hipError_t launch_tdm_step_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP, const TdmBuffers& TB,
                              int cur, const TdmIO& io, hipStream_t s);
hipError_t launch_tdm_init_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP, const TdmBuffers& TB,
                              int cur, void* obs, bool obs_f64, const uint8_t* mask, hipStream_t s);
hipError_t launch_tdm_observe_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                 const TdmBuffers& TB, void* obs, bool obs_f64, hipStream_t s);
// ---- tdm_obs_snap.hip, env_reset.hip, bots.hip, actions_check.hip
hipError_t launch_tdm_observe_snap(const TdmParams& TP, int N, size_t rows, const float4* snap, void* obs,
                                   bool obs_f64, uint8_t* mask, hipStream_t s);
hipError_t launch_draw_poses(const uint8_t* mask, uint32_t* mt, const PoseDraw& D, int n_envs, float2* pos,
                             float* angle, hipStream_t s);
hipError_t launch_final_copy(const uint8_t* mask, const FinalOut& F, const FinalRows& rows,
                             const int32_t* step_count, int n_envs, hipStream_t s);
hipError_t launch_bots_flock(const void* obs, bool obs_f64, int od, long long rows, uint8_t* act, hipStream_t s);
hipError_t launch_bots_combat(const void* obs, const uint8_t* mask, bool obs_f64, int N, long long rows,
                              uint8_t* act, hipStream_t s);
hipError_t launch_check_actions(const void* actions, int mode, const uint8_t* alive, long long rows,
                                unsigned long long* first_bad, hipStream_t s);
hipError_t launch_check_lists(const int32_t* count, const uint32_t* ab, int E, int C, int cap, int N,
                              unsigned long long* first_bad, hipStream_t s);

}  // namespace macm
