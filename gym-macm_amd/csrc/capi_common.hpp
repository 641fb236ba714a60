// capi_common.hpp — what the three units of the C-ABI of libmacm_hip.so share (capi_world.hip: Flock,
// capi_tdm.hip: TDM, capi_learn.hip: the stateless calls): the error path, the device guard and
// allocator, the step constants both env kinds derive, the host status word, and the checks and
// helpers that Flock and TDM worlds run alike. No torch types, no exceptions across the ABI.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "launch.hpp"
#include "ppo_row.hpp"
#include "py_mt19937.hpp"
#include "reward_threshold.h"

using namespace macm;

// macm_last_error's thread-local string lives in capi_learn.hip; every unit sets it through this
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(MACM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <typename T>
int dalloc(std::vector<void*>& allocs, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
  if (e != hipSuccess) return fail(MACM_E_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
  allocs.push_back(q);
  *p = (T*)q;
  return MACM_OK;
}

// Step constants shared by Flock and TDM, derived as the reference derives them.
inline void fill_body_params(StepParams& P, double hz, float radius, float density, float friction, float damping,
                             double agent_force, double rotation_speed) {
  // cm_framework.py:182-185 (timeStep = 1.0 / hz, a Python float) -> b2World::Step(float32 dt)
  volatile double dt64 = 1.0 / hz;
  P.dt = (float)dt64;
  P.inv_dt = 1.0f / P.dt;
  {
    // b2CircleShape::ComputeMass + b2Body::ResetMassData (settings.py:127-133)
    volatile float mass = density * kPi32 * radius * radius;
    P.inv_mass = mass > 0.0f ? 1.0f / mass : 1.0f;
    volatile float den = 1.0f + P.dt * damping;
    P.damp = 1.0f / den;
    volatile float ff = friction * friction;
    P.friction = sqrtf(ff);  // b2MixFriction
  }
  P.radius = radius;
  P.force_f32 = (float)agent_force;
  P.rot_step = rotation_speed;
  P.inv_hz = 1.0 / hz;
  P.force = agent_force;
  volatile double two = 2.0;
  P.diag_c = 1.0 / sqrt(two);  // 1 / np.sqrt(2)
}

// The host-mapped status word: kernels store nonzero status bits into it (report_status), and
// the step entry points read it without synchronising. Returns its device alias.
inline hipError_t alloc_host_status(uint32_t** host, uint32_t** dev) {
  hipError_t e = hipHostMalloc((void**)host, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return e;
  **host = 0u;
  return hipHostGetDevicePointer((void**)dev, *host, 0);
}

inline uint32_t read_host_status(const uint32_t* h) { return h ? __atomic_load_n(h, __ATOMIC_ACQUIRE) : 0u; }
inline void clear_host_status(uint32_t* h) {
  if (h) __atomic_store_n(h, 0u, __ATOMIC_RELEASE);
}

// After reset_envs: the init kernel rewrote the reset envs' status, so a set host word becomes the OR
// of what the envs still carry (0 once every overflowed env was reset; ADVICE r02: it kept the stale
// bits, and every later step failed). Only then does it synchronise the stream: with the word clear
// (the normal case, e.g. autoreset every step) reset_envs stays asynchronous.
inline int resync_host_status(uint32_t* h, const int32_t* dev_status, int E, hipStream_t s) {
  if (read_host_status(h) == 0u) return MACM_OK;
  std::vector<int32_t> st(E);
  HIP_TRY(hipMemcpyAsync(st.data(), dev_status, E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint32_t acc = 0u;
  for (int32_t v : st) acc |= (uint32_t)v;
  if (h) __atomic_store_n(h, acc, __ATOMIC_RELEASE);
  return MACM_OK;
}

// Default capacities (macm_world_create in include/macm.h), from a per-world memory budget of
// 1/8 of the device's free memory at creation (a fixed 8 GiB per world multiplied with
// the worlds or ranks sharing a device; every world now shrinks what the next one sees), half for
// the contact lists, half for the spill step's working set:
//   C = every pair when E * C * 24 B (two lists of pair + impulses) fits the lists' half (always
//       for N <= 64, the wave kernel), else the largest such C (at least 32 N);
//   S = spill working-set slots of 48 B per entry (C entries) + 48 B per body: one per env when
//       they fit the other half, else as many as fit (at least 16), taken by spilling envs in turn.
struct Capacity {
  int64_t C;
  int64_t slots;  // == E: one slot per env
};

// The most agents per env (Flock and TDM): one workgroup of 1024 threads, up to 4 bodies per thread
// (flock_big.hip, the spill step's BPT), 16-bit body ids in the lists (b < 32768 with a flag bit)
constexpr int kMaxAgents = 4096;

inline Capacity default_capacity(int N, int E, int64_t max_contacts, size_t free_bytes) {
  const int64_t all_pairs = (int64_t)N * (N - 1) / 2;
  const int64_t budget = std::max<int64_t>((int64_t)(free_bytes / 8), 256LL << 20);
  const int64_t half = budget / 2;
  Capacity cap;
  if (max_contacts > 0) cap.C = max_contacts;
  else if (N <= 64 || all_pairs * 24 * E <= half) cap.C = all_pairs;
  else cap.C = std::max<int64_t>(32LL * N, half / (24LL * E));
  cap.C = std::max<int64_t>(1, std::min(cap.C, all_pairs));
  const int64_t per_slot = cap.C * 48 + (int64_t)N * 48;
  cap.slots = std::min<int64_t>(E, std::max<int64_t>(16, half / per_slot));
  return cap;
}

// validate_actions (macm_config / macm_tdm_config): run the check kernel and wait for it.
// rows = n_steps * n_envs for a rollout's [K, E, N, A] actions; n_envs decodes the offending row
// into (step, env) (the env was reported as step * E + env)
inline int check_actions(unsigned long long* bad, const void* actions, int mode, const uint8_t* alive, int E, int N,
                         hipStream_t s, int n_envs = 0) {
  HIP_TRY(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
  HIP_TRY(launch_check_actions(actions, mode, alive, (long long)E * N, bad, s));
  unsigned long long h = ~0ull;
  HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h != ~0ull) {
    const char* space = mode == 0 ? "MultiDiscrete([3, 3, 3])" : mode == 1 ? "Box([-1, -1], [1, 1])"
                                                                           : "MultiDiscrete([3, 3, 3, 2])";
    const unsigned long long row = h / N;
    const std::string where = n_envs > 0 && (unsigned long long)E > (unsigned long long)n_envs
                                  ? "step " + std::to_string(row / n_envs) + " env " + std::to_string(row % n_envs)
                                  : "env " + std::to_string(row);
    return fail(MACM_E_INVALID, "action of " + where + " agent " + std::to_string(h % N) +
                                    " is not in the action space " + space + " (no env was stepped)");
  }
  return MACM_OK;
}

// Host generator state -> the env's slot of the device stream buffer.
inline void save_stream(std::vector<uint32_t>& host, int e, const PyMT19937& r) {
  uint32_t* d = host.data() + (size_t)e * kMtStride;
  memcpy(d, r.state(), sizeof(uint32_t) * PyMT19937::kWords);
  d[PyMT19937::kWords] = (uint32_t)r.index();
}

inline int fill_reset_mask(uint8_t* rmask, const uint8_t* env_mask, int E, hipStream_t s) {
  // a private copy: the init kernels clear the done flags a caller may pass as the mask
  if (env_mask) HIP_TRY(hipMemcpyAsync(rmask, env_mask, (size_t)E, hipMemcpyDefault, s));
  else HIP_TRY(hipMemsetAsync(rmask, 1, (size_t)E, s));
  return MACM_OK;
}

// The caller's final outputs as the kernels take them; `mask` / `nbr_id` as the env kind ignores them.
inline int final_outputs_from(const macm_final_outputs* fin, bool tdm, FinalOut* F) {
  *F = FinalOut{};
  if (!fin) return MACM_OK;
  if (reinterpret_cast<uintptr_t>(fin->obs) & 15)
    return fail(MACM_E_INVALID, "final outputs: obs must be 16-byte aligned");
  F->obs = fin->obs;
  F->nbr_id = tdm ? nullptr : fin->nbr_id;
  F->mask = tdm ? fin->mask : nullptr;
  F->length = fin->length;
  F->ends = fin->ends;
  return MACM_OK;
}

// An autoreset call copies a final row from the call's own output row: that row must exist. Checked
// before anything is launched.
inline int final_outputs_need(bool autoreset, const FinalOut& F, const void* obs, const void* nbr_id,
                              const void* mask) {
  if (!autoreset) return MACM_OK;
  if (F.obs && !obs) return fail(MACM_E_INVALID, "final outputs: obs is registered, so the call's obs output must be set");
  if (F.nbr_id && !nbr_id)
    return fail(MACM_E_INVALID, "final outputs: nbr_id is registered, so the call's nbr_id output must be set");
  if (F.mask && !mask)
    return fail(MACM_E_INVALID, "final outputs: mask is registered, so the call's mask output must be set");
  return MACM_OK;
}

inline int overflow_error(uint32_t st) {
  std::string what;
  if (st & MACM_ST_CONTACT_OVERFLOW) what += " contact-list capacity (max_contacts);";
  if (st & MACM_ST_TOUCH_OVERFLOW) what += " touching-contact capacity;";
  if (st & MACM_ST_DEGREE_OVERFLOW) what += " per-body contact capacity;";
  if (st & MACM_ST_SPILL_WAIT) what += " spill working-set pool (a dense env waited ~1 s for a slot);";
  if (st & MACM_ST_HANDOFF) what += " B -> C handoff (kernel B's waves did not all start, or a kernel-C block found no env, within ~1 s; every "
                                        "env is marked: rebuild the world or reset it);";
  return fail(MACM_E_OVERFLOW, "an env outgrew its" + what +
                                   " the results since that step are not the reference's (status bits " +
                                   std::to_string(st) + "; reset, place or set_state clears them)");
}

// Rows of E contact lists between the caller's [E, stride] layout and the world's [E, C] buffers:
// the first min(stride, C) entries of each row (the rest of a device row is never read, the rest
// of a caller's row is left as it is).
inline hipError_t copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t E,
                            hipStream_t s) {
  if (E == 0 || width == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, E, hipMemcpyDefault, s);
}

// set_state's contact lists: staged in the spare list buffer (cur ^ 1: the next step's output, unused
// between steps) and validated there on the device (a host loop over E x C entries).
// On success the caller flips its `cur` to take them; on failure nothing of the world changed.
inline int stage_lists(WorldBuffers& B, int cur, unsigned long long* bad, size_t E, size_t C, size_t Cs, int N,
                       const void* count, const void* ab, const void* imp, hipStream_t s) {
  const int nb = cur ^ 1;
  const size_t Cw = Cs < C ? Cs : C;
  HIP_TRY(hipMemcpyAsync(B.ccount[nb], count, E * sizeof(int32_t), hipMemcpyDefault, s));
  HIP_TRY(copy_rows(B.cab[nb], C * sizeof(uint32_t), ab, Cs * sizeof(uint32_t), Cw * sizeof(uint32_t), E, s));
  HIP_TRY(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
  HIP_TRY(launch_check_lists(B.ccount[nb], B.cab[nb], (int)E, (int)C, (int)Cw, N, bad, s));
  unsigned long long h = ~0ull;
  HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h != ~0ull) {
    const unsigned long long e = h >> 32, k = h & 0xffffffffull;
    if (k == 0xffffffffull)
      return fail(MACM_E_INVALID, "env " + std::to_string(e) + ": contact_count outside [0, min(max_contacts = " +
                                      std::to_string(C) + ", contact_stride = " + std::to_string(Cs) + ")]");
    return fail(MACM_E_INVALID, "env " + std::to_string(e) + ": contact_ab[" + std::to_string(k) +
                                    "] is not a pair a < b < n_agents");
  }
  if (imp)
    HIP_TRY(copy_rows(B.cimp[nb], C * sizeof(float2), imp, Cs * sizeof(float2), Cw * sizeof(float2), E, s));
  else
    HIP_TRY(hipMemsetAsync(B.cimp[nb], 0, E * C * sizeof(float2), s));
  return MACM_OK;
}

// The contact lists of macm_*_get_state / _set_state, for either world and state type. To the device:
// staged and validated (stage_lists), and the world's status cleared: an injected state starts clean.
template <typename Wt, typename St>
int copy_state_lists(Wt* w, const St* st, bool to_device, hipStream_t s) {
  const size_t E = w->P.n_envs, C = w->P.max_contacts;
  const size_t Cs = st->contact_stride > 0 ? (size_t)st->contact_stride : C;  // the caller's row length
  const size_t Cw = Cs < C ? Cs : C;                                           // entries moved per row
  if (!to_device) {
    if (st->contact_count)
      HIP_TRY(hipMemcpyAsync(st->contact_count, w->B.ccount[w->cur], E * sizeof(int32_t), hipMemcpyDefault, s));
    if (st->contact_ab)
      HIP_TRY(copy_rows(st->contact_ab, Cs * sizeof(uint32_t), w->B.cab[w->cur], C * sizeof(uint32_t),
                        Cw * sizeof(uint32_t), E, s));
    if (st->contact_imp)
      HIP_TRY(copy_rows(st->contact_imp, Cs * sizeof(float2), w->B.cimp[w->cur], C * sizeof(float2),
                        Cw * sizeof(float2), E, s));
    return MACM_OK;
  }
  if (!st->contact_count != !st->contact_ab)
    return fail(MACM_E_INVALID, "contact_count and contact_ab must be given together");
  if (st->contact_count) {
    const int rc = stage_lists(w->B, w->cur, w->bad, E, C, Cs, w->P.n_agents, st->contact_count, st->contact_ab,
                               st->contact_imp, s);
    if (rc) return rc;
    w->cur ^= 1;
  }
  HIP_TRY(hipStreamSynchronize(s));
  clear_host_status(w->hstat);
  HIP_TRY(hipMemsetAsync(w->B.status, 0, E * sizeof(int32_t), s));
  return MACM_OK;
}

// MACM_DEBUG_SPILL_POOL (a test hook): share `pool` of the slots allocated at creation;
// MACM_DEBUG_SPILL_FAIL: no slot is ever free (every spilling env ends SPILL_WAIT); a call
// without either flag brings back the world's own pool (or one slot per env). The locks are cleared
// only after the device has finished every step that could hold one.
template <typename Wt>
int set_spill_pool(Wt* w, int32_t flags, int pool) {
  const bool want = (flags & MACM_DEBUG_SPILL_POOL) != 0;
  const bool never = (flags & MACM_DEBUG_SPILL_FAIL) != 0;
  if (want && never) return fail(MACM_E_INVALID, "SPILL_POOL and SPILL_FAIL exclude each other");
  if (want && (pool < 1 || pool > w->slots_alloc))
    return fail(MACM_E_INVALID, "SPILL_POOL: 1 <= slots <= the " + std::to_string(w->slots_alloc) + " allocated");
  const int target = never ? -1 : want ? pool : w->pool0;  // -1: acquire_slot always fails
  if (target == w->B.sp_pool) return MACM_OK;
  DeviceGuard g(w->device);
  HIP_TRY(hipDeviceSynchronize());
  if (target > 0) {
    if (!w->B.sp_lock && dalloc(w->allocs, &w->B.sp_lock, (size_t)w->slots_alloc)) return MACM_E_OOM;
    HIP_TRY(hipMemset(w->B.sp_lock, 0, sizeof(uint32_t) * w->slots_alloc));
  }
  w->B.sp_pool = target;
  return MACM_OK;
}


// macm_world_status / macm_tdm_status, _counters and _spilled: the same body over either world type
template <typename Wt>
int world_status(Wt* w, int32_t* status_or, void* stream) {
  if (!w || !status_or) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  std::vector<int32_t> st(w->P.n_envs);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(st.data(), w->B.status, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int32_t acc = 0;
  for (int32_t v : st) acc |= v;
  *status_or = acc;
  return MACM_OK;
}

template <typename Wt>
int world_counters(Wt* w, int64_t out[4], void* stream) {
  if (!w || !out) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  std::vector<unsigned long long> h((size_t)w->P.n_envs * 4);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h.data(), w->B.env_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                         s));
  HIP_TRY(hipStreamSynchronize(s));
  unsigned long long acc[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < h.size(); ++i) acc[i & 3] += h[i];
  for (int i = 0; i < 4; ++i) out[i] = (int64_t)acc[i];
  return MACM_OK;
}

template <typename Wt>
int world_spilled(Wt* w, int64_t* env_steps, void* stream) {
  if (!w || !env_steps) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  std::vector<uint32_t> h((size_t)w->P.n_envs);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h.data(), w->B.spill_count, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int64_t acc = 0;
  for (uint32_t v : h) acc += v;
  *env_steps = acc;
  return MACM_OK;
}

// A policy or critic struct (macm_policy_mlp / macm_value_mlp; noun: "policy" / "critic") as the kernels
// can take it: shapes from the supported sets, params set and aligned
template <typename M>
int mlp_check(const std::string& noun, const M* m) {
  if (m->in_dim != 4 && m->in_dim != 6) return fail(MACM_E_INVALID, noun + ": in_dim must be 4 (polar) or 6 (cartesian)");
  if (m->hidden != 16 && m->hidden != 32) return fail(MACM_E_INVALID, noun + ": hidden must be 16 or 32");
  if (m->n_hidden != 1 && m->n_hidden != 2) return fail(MACM_E_INVALID, noun + ": n_hidden must be 1 or 2");
  if (m->reserved != 0) return fail(MACM_E_INVALID, noun + ": reserved must be 0");
  if (!m->params) return fail(MACM_E_INVALID, noun + ": params is NULL");
  if (reinterpret_cast<uintptr_t>(m->params) & 15) return fail(MACM_E_INVALID, noun + ": params must be 16-byte aligned");
  return MACM_OK;
}

// A macm_sample_config as the kernels can take it, over `rows` rows: the flat row is a 32-bit counter word
// starting at the job's row first_row (0: the entry points without _at)
inline int sample_check(const macm_sample_config* cfg, int64_t rows, int64_t first_row = 0) {
  constexpr int64_t kRowsEnd = (int64_t)1 << 32;
  if (!cfg) return fail(MACM_E_INVALID, "sampling: cfg is NULL");
  for (int i = 0; i < 4; ++i)
    if (cfg->reserved[i] != 0) return fail(MACM_E_INVALID, "sampling: reserved must be 0");
  if (rows < 0) return fail(MACM_E_INVALID, "sampling: rows must be >= 0");
  if (rows > kRowsEnd) return fail(MACM_E_INVALID, "sampling: rows must be <= 2^32 (the row is a 32-bit counter word)");
  if (first_row < 0) return fail(MACM_E_INVALID, "sampling: first_row must be >= 0");
  if (first_row > kRowsEnd || first_row + rows > kRowsEnd)  // (first_row <= 2^32 first: the sum cannot overflow)
    return fail(MACM_E_INVALID, "sampling: first_row + rows must be <= 2^32 (the row is a 32-bit counter word): first_row " +
                                    std::to_string(first_row) + ", rows " + std::to_string(rows));
  return MACM_OK;
}
