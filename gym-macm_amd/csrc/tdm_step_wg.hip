// tdm_step_wg.hip — TDM.step (gym_macm/envs/combat.py:104-184) for 64 < N <= 4096 agents per env:
// the reference takes any team sizes (combat.py:82-83) in an uncapped b2World (cm_framework.py:161);
// the wave kernel (flock_step_w64.hip, env_step_w64<kTdm>) holds one agent per lane, N <= 64.
//
// One workgroup per env, one thread per agent (blockDim = N rounded up to 64); above 1024 agents 1024
// threads with 2 or 4 agents each (round 5: the pair records then in HBM):
//   1. the action loop (combat.py:121-155) exactly as the wave kernel's: rotation (f32
//      SetTransform), force with the movement penalty, cooldowns, and the melee ray casts. Bodies do
//      not move during the loop and deaths come after it, so every cast sees the same world and all
//      rays are cast in parallel (candidates in body order, b2CircleShape::RayCast clipping the
//      fraction, as the oracle's b2l_world_raycast); only the shared listener's updates and the
//      damage are applied in agent order, by thread 0;
//   2. deaths (combat.py:157-165); the combat state is committed to HBM;
//   3. the physics, TDM.get_obs, done / winner by the spill step (flock_spill.hpp, MODE kTdm): the
//      touching-contact working set in HBM, the per-body arrays and pair records in LDS (88 B per
//      body: 88 KB at N = 1024), the observation in memory order (tdm_obs_block_linear).
// The spill step's arithmetic and order are those of the fast kernels, so results are bit-exact
// against the oracle (tests/test_gpu_tdm_wg.py). HBM per agent-step is dominated by the [N, N-1, 4]
// observation (16 (N-1) B at float32), as in the wave kernel.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <type_traits>

#include "flock_common.hpp"
#include "tdm_obs.hpp"
#include "flock_spill.hpp"
#include "launch.hpp"

namespace macm {
namespace tdmwg {

constexpr int W = 64;

__host__ __device__ constexpr int a16(int x) { return (x + 15) & ~15; }
__host__ __device__ constexpr int words(int N) { return (N + 31) / 32; }

// LDS of the action loop (dead when the spill step starts; it reuses the same bytes)
struct PreLayout {
  int c, hp, hit, aw, atw, total;
};
__host__ __device__ constexpr PreLayout pre_layout(int N) {
  PreLayout L{};
  int o = 0;
  L.c = o;  o = a16(o + 8 * N);            // float2 positions
  L.hp = o; o = a16(o + 8 * N);            // f64 health (damage applied in agent order)
  L.hit = o; o = a16(o + 4 * N);           // int32 ray hit of each attacker (-1: none)
  L.aw = o; o = a16(o + 4 * words(N));     // bitmap: alive at the step's start
  L.atw = o; o = a16(o + 4 * words(N));    // bitmap: attacking this step
  L.total = o;
  return L;
}

// the init / observe kernels' LDS: positions, angles, alive bitmap, fat AABBs, scan scratch
struct ObsLayout {
  int c, a, aw, fat, scan, total;
};
__host__ __device__ constexpr ObsLayout obs_layout(int N) {
  ObsLayout L{};
  int o = 0;
  L.c = o;  o = a16(o + 8 * N);
  L.a = o;  o = a16(o + 4 * N);
  L.aw = o; o = a16(o + 4 * words(N));
  L.fat = o; o = a16(o + 16 * N);
  L.scan = o; o = a16(o + 4 * 32);
  L.total = o;
  return L;
}

// wave w's ballot of body chunk j (bodies j BS + 64w ..) -> words 2 (j BS / 64 + w), + 1 of an LDS
// bitmap of N bits (call with the whole block)
__device__ __forceinline__ void ballot_bits(uint32_t* bits, int N, bool v, int j = 0) {
  const unsigned long long m = __ballot(v);
  const int tid = threadIdx.x;
  if ((tid & (W - 1)) == 0) {
    const int q = 2 * ((tid + j * (int)blockDim.x) / W);
    if (q < words(N)) bits[q] = (uint32_t)m;
    if (q + 1 < words(N)) bits[q + 1] = (uint32_t)(m >> 32);
  }
}

}  // namespace tdmwg

int tdm_wg_step_lds(int N) {
  // N > 1024 (BPT > 1): the pair records in HBM (spill step RECS_LDS = false)
  const int a = tdmwg::pre_layout(N).total, b = spill::layout(N, N <= 1024).total;
  return a > b ? a : b;
}
int tdm_wg_obs_lds(int N) { return tdmwg::obs_layout(N).total; }

// The step kernel, tdm_step_wg<OT, BPT>, and its twin that records the combat events, tdm_step_ev_wg
#define MACM_TDM_STEP_WG tdm_step_wg
#define MACM_TDM_STEP_WG_EV 0
#include "tdm_step_wg_kernel.inc"
#undef MACM_TDM_STEP_WG
#undef MACM_TDM_STEP_WG_EV
#define MACM_TDM_STEP_WG tdm_step_ev_wg
#define MACM_TDM_STEP_WG_EV 1
#include "tdm_step_wg_kernel.inc"
#undef MACM_TDM_STEP_WG
#undef MACM_TDM_STEP_WG_EV

// TDM world creation (combat.py:78-102) for N > 64: every body active with init_health, zero
// cooldowns, the fresh listener, fat AABBs and the first FindNewContacts list (every overlapping
// pair, a descending then b descending, as flock_init_wg), and the initial observation. The bodies in
// a loop (any N, any block size).
template <typename OT>
__global__ __launch_bounds__(1024) void tdm_init_wg(StepParams P, WorldBuffers B, TdmParams TP, TdmBuffers TB,
                                                    int cur, OT* __restrict__ obs, const uint8_t* __restrict__ mask) {
  using namespace tdmwg;
  extern __shared__ __align__(16) unsigned char lds[];
  const int e = blockIdx.x, tid = threadIdx.x, BS = blockDim.x, N = P.n_agents, C = P.max_contacts;
  if (mask && !mask[e]) return;  // reset_envs: only the masked envs
  const ObsLayout L = obs_layout(N);
  float2* s_c = (float2*)(lds + L.c);
  float* s_a = (float*)(lds + L.a);
  uint32_t* s_aw = (uint32_t*)(lds + L.aw);
  float4* s_f = (float4*)(lds + L.fat);
  int* s_scan = (int*)(lds + L.scan);
  for (int i = tid; i < N; i += BS) {
    const size_t ag = (size_t)e * N + i;
    const float2 p = B.pos[ag];
    const float r = P.radius;
    const float4 f = make_float4((p.x - r) - kAabbExtension, (p.y - r) - kAabbExtension, (p.x + r) + kAabbExtension,
                                 (p.y + r) + kAabbExtension);
    B.fat[ag] = f;
    B.vel[ag] = make_float2(0.0f, 0.0f);
    B.sleep[ag] = 0.0f;
    TB.health[ag] = TP.init_health;
    TB.cd_atk[ag] = 0.0;
    TB.cd_mov[ag] = 0.0;
    TB.alive[ag] = 1;
    if (TB.health_out) TB.health_out[ag] = TP.init_health;
    if (TB.alive_out) TB.alive_out[ag] = 1;
    s_c[i] = p;
    s_a[i] = B.angle[ag];
    s_f[i] = f;
  }
  for (int q = tid; q < words(N); q += BS) s_aw[q] = q + 1 < words(N) || N % 32 == 0 ? ~0u : (1u << (N % 32)) - 1u;
  __syncthreads();
  // pairs in (a desc, b desc) order: chunks of BS bodies in body order, the total first
  int total = 0;
  for (int i0 = 0; i0 < N; i0 += BS) {
    const int i = i0 + tid;
    int cnt = 0;
    if (i < N)
      for (int j = i + 1; j < N; ++j) cnt += spill::overlap(s_f[i], s_f[j]) ? 1 : 0;
    int excl;
    total += spill::block_scan_excl(cnt, excl, s_scan);
  }
  int base = 0;
  for (int i0 = 0; i0 < N; i0 += BS) {
    const int i = i0 + tid;
    int cnt = 0;
    if (i < N)
      for (int j = i + 1; j < N; ++j) cnt += spill::overlap(s_f[i], s_f[j]) ? 1 : 0;
    int excl;
    const int tot = spill::block_scan_excl(cnt, excl, s_scan);
    if (i < N && cnt > 0) {
      int w = total - (base + excl) - cnt;  // agents > i come first
      for (int j = N - 1; j > i; --j)
        if (spill::overlap(s_f[i], s_f[j])) {
          if (w < C) {
            B.cab[cur][(size_t)e * C + w] = (uint32_t)i | ((uint32_t)j << 16);
            B.cimp[cur][(size_t)e * C + w] = make_float2(0.0f, 0.0f);
          }
          ++w;
        }
    }
    base += tot;
  }
  const size_t rows = (size_t)e * N * (N - 1);
  for (int i = tid; i - tid < N; i += BS)  // tdm_obs_block returns for i >= N
    tdm_obs_block<OT>(obs ? obs + rows * 4 : nullptr, TB.mask_out ? TB.mask_out + rows : nullptr, N, i, s_aw, TP,
                      s_c, s_a);
  if (tid == 0) {
    const int st = total > C ? MACM_ST_CONTACT_OVERFLOW : 0;
    B.ccount[cur][e] = total > C ? C : total;
    B.step_count[e] = 0;
    B.time_passed[e] = 0.0;
    B.done[e] = 0;
    B.status[e] = st;
    if (st) report_status(B, st);
    TB.listener[e] = make_int2(0, -1);
    TB.winner[e] = -1;
    if (TB.winner_out) TB.winner_out[e] = -1;
  }
}

// TDM.get_obs of the current state without stepping (N > 64; the bodies in a loop).
template <typename OT>
__global__ __launch_bounds__(1024) void tdm_observe_wg(StepParams P, WorldBuffers B, TdmParams TP, TdmBuffers TB,
                                                       OT* __restrict__ obs) {
  using namespace tdmwg;
  extern __shared__ __align__(16) unsigned char lds[];
  const int e = blockIdx.x, tid = threadIdx.x, BS = blockDim.x, N = P.n_agents;
  const ObsLayout L = obs_layout(N);
  float2* s_c = (float2*)(lds + L.c);
  float* s_a = (float*)(lds + L.a);
  uint32_t* s_aw = (uint32_t*)(lds + L.aw);
  for (int i0 = 0, j = 0; i0 < N; i0 += BS, ++j) {
    const int i = i0 + tid;
    const size_t ag = (size_t)e * N + i;
    bool live = false;
    if (i < N) {
      s_c[i] = B.pos[ag];
      s_a[i] = B.angle[ag];
      live = TB.alive[ag] != 0;
    }
    ballot_bits(s_aw, N, live, j);
  }
  __syncthreads();
  const size_t rows = (size_t)e * N * (N - 1);
  for (int i = tid; i - tid < N; i += BS)
    tdm_obs_block<OT>(obs ? obs + rows * 4 : nullptr, TB.mask_out ? TB.mask_out + rows : nullptr, N, i, s_aw, TP,
                      s_c, s_a);
}

// ---- host-side launchers (declared in launch.hpp) --------------------------------------------------
static int tdm_wg_block(int N) { return N > 1024 ? 1024 : ((N + 63) / 64) * 64; }

// as wg_configure: the kernels' dynamic-LDS limits only grow (per device)
hipError_t tdm_wg_configure(int N) {
  static std::mutex mu;
  static std::map<int, int> high;
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  int& hw = high[dev];
  if (N <= hw) return hipSuccess;
  hw = N;
  const int ls = tdm_wg_step_lds(N), lo = tdm_wg_obs_lds(N);
  const void* fs[] = {(const void*)tdm_step_wg<float>, (const void*)tdm_step_wg<double>,
                      (const void*)tdm_step_wg<float, 2>, (const void*)tdm_step_wg<double, 2>,
                      (const void*)tdm_step_wg<float, 4>, (const void*)tdm_step_wg<double, 4>,
                      (const void*)tdm_step_ev_wg<float>, (const void*)tdm_step_ev_wg<double>,
                      (const void*)tdm_step_ev_wg<float, 2>, (const void*)tdm_step_ev_wg<double, 2>,
                      (const void*)tdm_step_ev_wg<float, 4>, (const void*)tdm_step_ev_wg<double, 4>};
  const void* fo[] = {(const void*)tdm_init_wg<float>, (const void*)tdm_init_wg<double>,
                      (const void*)tdm_observe_wg<float>, (const void*)tdm_observe_wg<double>};
  hipError_t e = hipSuccess;
  for (const void* f : fs)
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, ls);
  for (const void* f : fo)
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lo);
  return e;
}

hipError_t launch_tdm_step_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP, const TdmBuffers& TB,
                              int cur, const TdmIO& io, hipStream_t s) {
  const dim3 grid(P.n_envs), block(tdm_wg_block(P.n_agents));
  const int lds = tdm_wg_step_lds(P.n_agents);
  const uchar4* a = (const uchar4*)io.actions;
  // bodies per thread 1, 2 or 4; events registered: the kernels that record them
  const auto go = [&](auto ot, auto bpt) {
    using OT = decltype(ot);
    constexpr int BPT = decltype(bpt)::value;
    if (io.hit_out)
      hipLaunchKernelGGL((tdm_step_ev_wg<OT, BPT>), grid, block, lds, s, P, B, TP, TB, cur, a, (OT*)io.obs, io.done,
                         io.hit_out);
    else
      hipLaunchKernelGGL((tdm_step_wg<OT, BPT>), grid, block, lds, s, P, B, TP, TB, cur, a, (OT*)io.obs, io.done);
  };
  with_obs_type(io.obs_f64, [&](auto ot) {
    if (P.n_agents <= 1024) go(ot, std::integral_constant<int, 1>{});
    else if (P.n_agents <= 2048) go(ot, std::integral_constant<int, 2>{});
    else go(ot, std::integral_constant<int, 4>{});
  });
  return hipGetLastError();
}

hipError_t launch_tdm_init_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP, const TdmBuffers& TB,
                              int cur, void* obs, bool obs_f64, const uint8_t* mask, hipStream_t s) {
  const dim3 grid(P.n_envs), block(tdm_wg_block(P.n_agents));
  const int lds = tdm_wg_obs_lds(P.n_agents);
  with_obs_type(obs_f64, [&](auto ot) {
    hipLaunchKernelGGL(tdm_init_wg<decltype(ot)>, grid, block, lds, s, P, B, TP, TB, cur, (decltype(ot)*)obs, mask);
  });
  return hipGetLastError();
}

hipError_t launch_tdm_observe_wg(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                 const TdmBuffers& TB, void* obs, bool obs_f64, hipStream_t s) {
  const dim3 grid(P.n_envs), block(tdm_wg_block(P.n_agents));
  const int lds = tdm_wg_obs_lds(P.n_agents);
  with_obs_type(obs_f64, [&](auto ot) {
    hipLaunchKernelGGL(tdm_observe_wg<decltype(ot)>, grid, block, lds, s, P, B, TP, TB, (decltype(ot)*)obs);
  });
  return hipGetLastError();
}

}  // namespace macm
