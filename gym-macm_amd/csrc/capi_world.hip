// capi_world.hip — the Flock worlds of the C-ABI of libmacm_hip.so (declared in include/macm.h).
//
// Owns the per-world device state (SoA, sized for E envs x N agents), derives the step constants from
// macm_config the way the reference derives them, seeds envs with the reference's RNG order, and
// launches the HIP kernels on the caller's stream. No torch types, no exceptions across the ABI.
#include "capi_common.hpp"

struct macm_world {
  macm_config cfg;
  StepParams P;
  WorldBuffers B;
  int cur;  // which contact-list buffer holds the current ordered list
  int device;
  bool wave;  // N <= 64: one wavefront per env (flock_step_w64); else one workgroup per env
  bool big;   // N > 1024: the spill step with several bodies per thread (flock_big.hip)
  int tcap;   // touching-contact capacity per env of the fast kernels (more: the spill step)
  std::vector<int32_t> tidx;
  std::vector<void*> allocs;
  uint32_t* mt = nullptr;     // [E][kMtStride] per-env MT19937 streams (valid after reset)
  uint8_t* rmask = nullptr;   // [E] reset mask scratch
  bool mt_valid = false;
  bool autoreset = false;     // macm_world_set_autoreset: step and rollouts restart the envs that end
  FinalOut fin{};             // macm_world_set_final_outputs: the caller's buffers, kept until replaced or cleared
  // macm_world_set_policy: the caller's params buffer, kept until replaced or cleared (params NULL: none)
  macm_policy_mlp policy{0, 0, 0, 0, nullptr};
  macm_value_mlp critic{0, 0, 0, 0, nullptr};  // macm_world_set_critic: likewise
  // macm_world_set_sampling: the policy rollouts draw their own noise; sample.decision is the next launch's first
  bool sampling = false;
  SampleArgs sample{0, 0, 0};
  uint32_t* hstat = nullptr;  // host-mapped status word (B.host_status is its device alias)
  unsigned long long* bad = nullptr;  // validate_actions: first failing row (device scratch)
  // workgroup-path rollouts: env slices on streams of their own (created on first use)
  std::vector<hipStream_t> slice_streams;
  std::vector<hipEvent_t> slice_events;  // [0] fork, [1 + s] join of slice s
  HandoffStream* ho = nullptr;  // workgroup path: kernel C as kernel B's consumer (handoff_for)
  bool ho_tried = false;
  int slots_alloc = 0;  // spill working-set slots allocated (== E: one per env)
  int pool0 = 0;        // B.sp_pool as created (0: one slot per env), restored by set_debug
  // wave rollouts: bit 0 MACM_DEBUG_ROLLOUT_RELOAD (load and fence every step), bit 1 MACM_DEBUG_NEAR_PLAIN
  // (the plain nearest-neighbour sweep every step)
  int roll_reload = 0;
};

namespace {

int obs_dim(const macm_config& c) { return c.coord == MACM_COORD_CARTESIAN ? 6 : 4; }

static void free_handoff(HandoffStream*& h) {
  if (!h) return;
  if (h->stream) (void)hipStreamDestroy(h->stream);
  if (h->done) (void)hipEventDestroy(h->done);
  if (h->pre_b) (void)hipEventDestroy(h->pre_b);
  if (h->b_started) (void)hipFree(h->b_started);
  if (h->ctr) (void)hipFree(h->ctr);
  if (h->q) (void)hipFree(h->q);
  delete h;
  h = nullptr;
}

void free_world(macm_world* w) {
  free_handoff(w->ho);
  for (hipStream_t st : w->slice_streams) (void)hipStreamDestroy(st);
  for (hipEvent_t ev : w->slice_events) (void)hipEventDestroy(ev);
  w->slice_streams.clear();
  w->slice_events.clear();
  for (void* p : w->allocs) (void)hipFree(p);
  w->allocs.clear();
  if (w->hstat) (void)hipHostFree(w->hstat);
  w->hstat = nullptr;
}

// the end of a world: macm_world_destroy, and macm_world_create's failure paths
int drop_world(macm_world* w, int rc) {
  free_world(w);
  delete w;
  return rc;
}

// Kernel dispatches run one at a time: HIP's serialisation switches, or a profiler collecting counters
// (rocprofv3 --pmc serialises dispatches to attribute counters to them). The producer/consumer
// launch pair of the B -> C handoff needs its consumer to run BESIDE the producer: under
// serialisation the consumer's wait would time out and the step be left incomplete, so it is off.
static bool serialized_dispatch() {
  for (const char* k : {"AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING"}) {
    const char* v = getenv(k);
    if (v && atoi(v) != 0) return true;
  }
  const char* pmc = getenv("ROCPROF_COUNTER_COLLECTION");
  return pmc && *pmc && strcmp(pmc, "0") != 0 && strcasecmp(pmc, "false") != 0;
}

hipError_t launch_init(macm_world* w, const macm_outputs* out, const uint8_t* mask, hipStream_t s) {
  void* obs = out ? out->obs : nullptr;
  int32_t* nbr = out ? out->nbr_id : nullptr;
  if (w->wave) return launch_init_w64(w->P, w->B, w->cur, obs, w->cfg.obs_f64 != 0, nbr, mask, s);
  if (w->big) return launch_init_big(w->P, w->B, w->cur, obs, w->cfg.obs_f64 != 0, nbr, mask, s);
  return launch_init_wg(w->P, w->B, w->cur, obs, w->cfg.obs_f64 != 0, nbr, mask, s);
}

}  // namespace

extern "C" {

int macm_config_default(macm_config* c) {
  if (!c) return fail(MACM_E_INVALID, "cfg is NULL");
  memset(c, 0, sizeof(*c));
  c->n_agents = 10;  // Flock(n_agents=[10]) default, mvmnt.py:35
  c->n_targets = 1;
  c->action_mode = MACM_ACTION_DISCRETE;
  c->reward_mode = MACM_REWARD_BINARY;
  c->coord = MACM_COORD_POLAR;
  c->velocity_iterations = 8;
  c->position_iterations = 3;
  c->warm_starting = 1;
  c->obs_f64 = 0;
  c->hz = 60.0;
  c->start_spread = 20.0;
  c->start_point[0] = 0.0;
  c->start_point[1] = 0.0;
  c->agent_rotation_speed = 0.8 * (2 * M_PI);
  c->agent_force = 20.0;
  c->time_limit = 60.0;
  c->reward_radius = 7.0;
  c->target_mindist = 25.0;
  c->target_maxdist = 60.0;
  c->radius = 0.5f;
  c->density = 1.0f;
  c->friction = 0.3f;
  c->linear_damping = 5.0f;
  return MACM_OK;
}

int macm_world_create(const macm_config* cfg, const int32_t* targets_idx, int32_t n_envs, int32_t device,
                      int32_t max_contacts, macm_world** out) {
  if (!cfg || !out) return fail(MACM_E_INVALID, "cfg/out is NULL");
  *out = nullptr;
  const macm_config& c = *cfg;
  if (n_envs <= 0) return fail(MACM_E_INVALID, "n_envs must be > 0");
  if (c.n_agents < 2) return fail(MACM_E_INVALID, "n_agents must be >= 2 (get_obs needs another agent)");
  if (c.n_agents > kMaxAgents)
    return fail(MACM_E_UNSUPPORTED, "n_agents > 4096 is not built (one workgroup per env, <= 4 bodies per thread)");
  if (c.n_targets < 1) return fail(MACM_E_INVALID, "n_targets must be >= 1");
  if (!(c.hz > 0.0)) return fail(MACM_E_INVALID, "hz must be > 0");
  if (c.velocity_iterations < 0 || c.position_iterations < 0) return fail(MACM_E_INVALID, "iterations < 0");
  if (c.action_mode != MACM_ACTION_DISCRETE && c.action_mode != MACM_ACTION_CONTINUOUS)
    return fail(MACM_E_INVALID, "action_mode");
  if (c.reward_mode != MACM_REWARD_BINARY && c.reward_mode != MACM_REWARD_LINEAR)
    return fail(MACM_E_INVALID, "reward_mode");
  if (c.coord != MACM_COORD_POLAR && c.coord != MACM_COORD_CARTESIAN) return fail(MACM_E_INVALID, "coord");
  if (!(c.radius > 0.0f)) return fail(MACM_E_INVALID, "radius must be > 0");
  const int N = c.n_agents, T = c.n_targets;
  std::vector<int32_t> tidx(N, 0);
  if (targets_idx)
    for (int i = 0; i < N; ++i) {
      if (targets_idx[i] < 0 || targets_idx[i] >= T) return fail(MACM_E_INVALID, "targets_idx out of range");
      tidx[i] = targets_idx[i];
    }
  if (max_contacts < 0) return fail(MACM_E_INVALID, "max_contacts must be >= 0");

  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MACM_E_INVALID, "device index out of range");
  DeviceGuard g(device);
  size_t free_bytes = 0, total_bytes = 0;
  HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
  const Capacity cap = default_capacity(N, n_envs, max_contacts, free_bytes);
  const int C = (int)cap.C;
  const int64_t SL = cap.slots;  // spill working-set slots

  macm_world* w = new macm_world();
  w->cfg = c;
  w->device = device;
  w->cur = 0;
  w->tidx = tidx;
  w->wave = N <= 64;
  w->big = N > 1024;  // flock_big.hip: the spill step with several bodies per thread
  {
    const int bs = N <= 64 ? 64 : wg_block(N);
    const int want = N <= 64 ? 256 : 5 * bs;  // register staging holds 5 records per thread
    w->tcap = w->big ? C : want < 4608 ? want : 4608;  // big: every touching contact takes the spill step
  }
  StepParams& P = w->P;
  P.n_envs = n_envs;
  P.n_agents = N;
  P.n_targets = T;
  P.max_contacts = C;
  P.vel_iters = c.velocity_iterations;
  P.pos_iters = c.position_iterations;
  P.warm_starting = c.warm_starting ? 1 : 0;
  P.action_mode = c.action_mode;
  P.reward_mode = c.reward_mode;
  P.coord = c.coord;
  P.force_spill = 0;
  P.sweep = 0;
  fill_body_params(P, c.hz, c.radius, c.density, c.friction, c.linear_damping, c.agent_force,
                   c.agent_rotation_speed);
  P.reward_radius = c.reward_radius;
  P.reward_thr2 = macm_reward_thr2(c.reward_radius);
  P.time_limit = c.time_limit;

  WorldBuffers& B = w->B;
  memset(&B, 0, sizeof(B));
  const size_t EN = (size_t)n_envs * N;
  std::vector<void*>& A = w->allocs;
  int rc = MACM_OK;
  if ((rc = dalloc(A, &B.pos, EN)) || (rc = dalloc(A, &B.vel, EN)) || (rc = dalloc(A, &B.angle, EN)) ||
      (rc = dalloc(A, &B.fat, EN)) || (rc = dalloc(A, &B.sleep, EN)) ||
      (rc = dalloc(A, &B.targets, (size_t)n_envs * T)) || (rc = dalloc(A, &B.tidx, (size_t)N)) ||
      (rc = dalloc(A, &B.ccount[0], (size_t)n_envs)) || (rc = dalloc(A, &B.ccount[1], (size_t)n_envs)) ||
      (rc = dalloc(A, &B.cab[0], (size_t)n_envs * C)) || (rc = dalloc(A, &B.cab[1], (size_t)n_envs * C)) ||
      (rc = dalloc(A, &B.cimp[0], (size_t)n_envs * C)) || (rc = dalloc(A, &B.cimp[1], (size_t)n_envs * C)) ||
      (rc = dalloc(A, &B.step_count, (size_t)n_envs)) || (rc = dalloc(A, &B.time_passed, (size_t)n_envs)) ||
      (rc = dalloc(A, &B.done, (size_t)n_envs)) || (rc = dalloc(A, &B.status, (size_t)n_envs)) ||
      (rc = dalloc(A, &B.env_counters, (size_t)n_envs * 4)) || (rc = dalloc(A, &B.env_rsum, (size_t)n_envs))
#ifdef MACM_STAMPS
      || (rc = dalloc(A, &B.stamps, (size_t)n_envs * 32))
#endif
      || (!w->wave && !w->big && (rc = dalloc(A, &B.scratch, (size_t)n_envs * w->tcap))) ||
      (!w->wave && !w->big && ((rc = dalloc(A, &B.x_cst, (size_t)n_envs * w->tcap)) ||
                    (rc = dalloc(A, &B.x_cimp, (size_t)n_envs * w->tcap)) ||
                    (rc = dalloc(A, &B.x_ord, (size_t)n_envs * w->tcap)) ||
                    (rc = dalloc(A, &B.x_ic, (size_t)n_envs * (N / 2 + 2))) ||
                    (rc = dalloc(A, &B.x_nlvl, (size_t)n_envs)) ||
                    (rc = dalloc(A, &B.x_ib, (size_t)n_envs * (N / 2 + 2))) ||
                    (rc = dalloc(A, &B.x_ibod, EN)) || (rc = dalloc(A, &B.x_nisl, (size_t)n_envs)) ||
                    (rc = dalloc(A, &B.x_vmid, EN)) || (rc = dalloc(A, &B.x_cout, EN)) ||
                    (rc = dalloc(A, &B.x_vout, EN)) || (rc = dalloc(A, &B.x_deg, EN)) ||
                    (rc = dalloc(A, &B.x_isolv, (size_t)n_envs * (N / 2 + 2))) ||
                    (rc = dalloc(A, &B.x_tab, (size_t)n_envs * w->tcap)) ||
                    (rc = dalloc(A, &B.x_adj, (size_t)n_envs * 2 * w->tcap)) ||
                    (rc = dalloc(A, &B.x_off, (size_t)n_envs * (N + 1))) ||
                    (rc = dalloc(A, &B.x_dfs, (size_t)n_envs * w->tcap)))) ||
      // spill step working set (flock_spill.hpp), capacity C per slot, SL slots
      (rc = dalloc(A, &B.sp_tab, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_adj, (size_t)SL * 2 * C)) ||
      (rc = dalloc(A, &B.sp_ord, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_cst, (size_t)SL * C)) ||
      (rc = dalloc(A, &B.sp_cim, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_lam, (size_t)SL * C)) ||
      (!w->wave && (rc = dalloc(A, (float4**)&B.sp_rec, (size_t)SL * N * 3))) ||  // 48-B records
      (SL < n_envs && (rc = dalloc(A, &B.sp_lock, (size_t)SL))) ||
      (rc = dalloc(A, &B.spill_count, (size_t)n_envs)) || (rc = dalloc(A, &w->bad, 1)) ||
      (rc = dalloc(A, &B.sched, (size_t)n_envs)) ||
      (rc = dalloc(A, &w->mt, (size_t)n_envs * kMtStride)) || (rc = dalloc(A, &w->rmask, (size_t)n_envs))
  )
    return drop_world(w, rc);
  if (hipError_t he = alloc_host_status(&w->hstat, &B.host_status); he != hipSuccess)
    return drop_world(w, fail(MACM_E_OOM, std::string("hipHostMalloc (status word): ") + hipGetErrorString(he)));
  hipError_t e = hipMemcpy(B.tidx, tidx.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(B.env_counters, 0, (size_t)n_envs * 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(B.env_rsum, 0, (size_t)n_envs * sizeof(double));
  if (e == hipSuccess) e = hipMemset(B.ccount[0], 0, sizeof(int32_t) * n_envs);
  if (e == hipSuccess) e = hipMemset(B.status, 0, sizeof(int32_t) * n_envs);
  if (e == hipSuccess) e = hipMemset(B.spill_count, 0, sizeof(uint32_t) * n_envs);
  B.sp_pool = SL < n_envs ? (int32_t)SL : 0;
  w->slots_alloc = (int)SL;
  w->pool0 = B.sp_pool;
  if (e == hipSuccess && B.sp_lock) e = hipMemset(B.sp_lock, 0, sizeof(uint32_t) * SL);
  if (e == hipSuccess && w->big) {
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess && (size_t)std::max(big_step_lds(N), big_init_lds(N)) > prop.sharedMemPerBlock)
      return drop_world(w, fail(MACM_E_UNSUPPORTED, "per-env LDS layout exceeds the device's LDS per workgroup"));
    if (e == hipSuccess) e = big_configure(N);
  } else if (e == hipSuccess && !w->wave) {
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess && (size_t)wg_lds_bytes(N, w->tcap) > prop.sharedMemPerBlock)
      return drop_world(w, fail(MACM_E_UNSUPPORTED, "per-env LDS layout exceeds the device's LDS per workgroup"));
    if (e == hipSuccess) e = wg_configure(N, w->tcap);
  }
  if (e != hipSuccess) return drop_world(w, fail(MACM_E_HIP, std::string("world init copy: ") + hipGetErrorString(e)));
  *out = w;
  return MACM_OK;
}

int macm_world_destroy(macm_world* w) {
  if (!w) return MACM_OK;
  DeviceGuard g(w->device);
  (void)hipDeviceSynchronize();
  return drop_world(w, MACM_OK);
}

static int wg_rollout_slices(const macm_world* w);

int macm_world_info_get(const macm_world* w, macm_world_info* info) {
  if (!w || !info) return fail(MACM_E_INVALID, "NULL argument");
  info->n_envs = w->P.n_envs;
  info->n_agents = w->P.n_agents;
  info->n_targets = w->P.n_targets;
  info->obs_dim = obs_dim(w->cfg);
  info->max_contacts = w->P.max_contacts;
  info->max_touching = w->tcap;
  info->device = w->device;
  info->spill_slots = w->B.sp_pool > 0 ? w->B.sp_pool : w->P.n_envs;
  info->launch_flags = w->ho ? MACM_LAUNCH_HANDOFF : 0;
  info->rollout_slices = wg_rollout_slices(w);
  return MACM_OK;
}

int macm_world_reset(macm_world* w, uint64_t seed, int64_t env_offset, const macm_outputs* out, void* stream) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  DeviceGuard g(w->device);
  const macm_config& c = w->cfg;
  const int E = w->P.n_envs, N = w->P.n_agents, T = w->P.n_targets;
  std::vector<float2> pos((size_t)E * N), tg((size_t)E * T);
  std::vector<float> ang((size_t)E * N);
  std::vector<uint32_t> mts((size_t)E * kMtStride);
  for (int e = 0; e < E; ++e) {
    PyMT19937 r(seed + (uint64_t)(env_offset + e));
    for (int t = 0; t < T; ++t) {  // mvmnt.py:46-52
      const double rand_angle = 2 * M_PI * r.random();
      const double rand_dist = c.target_mindist + r.random() * (c.target_maxdist - c.target_mindist);
      tg[(size_t)e * T + t] = make_float2((float)(rand_dist * cos(rand_angle)), (float)(rand_dist * sin(rand_angle)));
    }
    for (int i = 0; i < N; ++i) {  // mvmnt.py:61-64, CreateDynamicBody(position=(x, y), angle=angle)
      const double x = c.start_spread * (r.random() - 0.5) + c.start_point[0];
      const double y = c.start_spread * (r.random() - 0.5) + c.start_point[1];
      const double a = r.uniform(-1, 1) * M_PI;
      pos[(size_t)e * N + i] = make_float2((float)x, (float)y);
      ang[(size_t)e * N + i] = (float)a;
    }
    save_stream(mts, e, r);
  }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipStreamSynchronize(s));  // earlier steps' status stores land before the word is cleared
  clear_host_status(w->hstat);
  HIP_TRY(hipMemcpyAsync(w->B.pos, pos.data(), pos.size() * sizeof(float2), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(w->B.angle, ang.data(), ang.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(w->B.targets, tg.data(), tg.size() * sizeof(float2), hipMemcpyHostToDevice, s));
  w->cur = 0;
  HIP_TRY(hipMemcpyAsync(w->mt, mts.data(), mts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  w->mt_valid = true;
  HIP_TRY(launch_init(w, out, nullptr, s));
  // host vectors are read by the async copies: wait before they go out of scope
  HIP_TRY(hipStreamSynchronize(s));
  return MACM_OK;
}

int macm_world_place(macm_world* w, const void* pos, const void* angle, const void* targets,
                     const macm_outputs* out, void* stream) {
  if (!w || !pos || !angle || !targets) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  const size_t EN = (size_t)w->P.n_envs * w->P.n_agents, ET = (size_t)w->P.n_envs * w->P.n_targets;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipStreamSynchronize(s));
  clear_host_status(w->hstat);
  HIP_TRY(hipMemcpyAsync(w->B.pos, pos, EN * sizeof(float2), hipMemcpyDefault, s));
  HIP_TRY(hipMemcpyAsync(w->B.angle, angle, EN * sizeof(float), hipMemcpyDefault, s));
  HIP_TRY(hipMemcpyAsync(w->B.targets, targets, ET * sizeof(float2), hipMemcpyDefault, s));
  w->cur = 0;
  w->mt_valid = false;  // poses came from the caller's generator
  HIP_TRY(launch_init(w, out, nullptr, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MACM_OK;
}

static const char* const kNoStreams = "no per-env random streams: the world was placed, not reset (macm_world_reset)";

static PoseDraw world_pose_draw(const macm_world* w) {
  PoseDraw D;
  memset(&D, 0, sizeof(D));
  D.mode = kFlock;
  D.n_agents = w->P.n_agents;
  D.spread = w->cfg.start_spread;
  D.start_x = w->cfg.start_point[0];
  D.start_y = w->cfg.start_point[1];
  return D;
}

// the draw and init launches of the envs masked in w->rmask (the new initial obs / nbr_id into `out`)
static int world_reset_masked(macm_world* w, const macm_outputs* out, hipStream_t s) {
  HIP_TRY(launch_draw_poses(w->rmask, w->mt, world_pose_draw(w), w->P.n_envs, w->B.pos, w->B.angle, s));
  HIP_TRY(launch_init(w, out, w->rmask, s));
  return MACM_OK;
}

int macm_world_reset_envs(macm_world* w, const uint8_t* env_mask, const macm_outputs* out, void* stream) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  if (!w->mt_valid) return fail(MACM_E_INVALID, kNoStreams);
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = fill_reset_mask(w->rmask, env_mask, w->P.n_envs, s);
  if (rc) return rc;
  if ((rc = world_reset_masked(w, out, s))) return rc;
  return resync_host_status(w->hstat, w->B.status, w->P.n_envs, s);
}

int macm_world_set_autoreset(macm_world* w, int32_t on) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  w->autoreset = on != 0;
  return MACM_OK;
}

// Autoreset after a step's launches (macm_world_step, and every step of a workgroup-path rollout):
// the step's done flags, as a private copy (the init kernel clears B.done; the output row keeps its
// 1), mask the draw and init launches. All on the stream, no host round trip; the host-mapped
// status word is not resynced here.
// With final outputs registered, the rows the init is about to overwrite are copied out first
// (final_copy_kernel, the same mask), launched only then.
static int world_autoreset_step(macm_world* w, const macm_outputs* out, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(w->rmask, w->B.done, (size_t)w->P.n_envs, hipMemcpyDeviceToDevice, s));
  if (w->fin.any()) {
    const unsigned long long obytes =
        (unsigned long long)w->P.n_agents * obs_dim(w->cfg) * (w->cfg.obs_f64 ? sizeof(double) : sizeof(float));
    FinalRows rows;
    rows.obs = out->obs;
    rows.obs_bytes = obytes;
    rows.nbr = out->nbr_id;
    rows.n_nbr = w->P.n_agents;
    HIP_TRY(launch_final_copy(w->rmask, w->fin, rows, w->B.step_count, w->P.n_envs, s));
  }
  return world_reset_masked(w, out, s);
}

int macm_world_set_final_outputs(macm_world* w, const macm_final_outputs* fin) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  FinalOut F;
  const int rc = final_outputs_from(fin, false, &F);
  if (rc) return rc;
  w->fin = F;
  return MACM_OK;
}

// The workgroup step's B -> C handoff (flock_common.hpp Handoff), created at the first step that can
// use it: the workgroup path, when kHandoffDefault or MACM_HANDOFF=1 (A/B; MACM_HANDOFF=0 off). Env
// slices (rollout_wg_slices) run without it. NULL: kernel C launched after B on the same stream.
static constexpr bool kHandoffDefault = true;  // round 5: C5 window 5.35 -> 4.99 ms (profiles/r05/abtests/handoff_fused/)
static HandoffStream* handoff_for(macm_world* w) {
  if (w->wave || w->big || w->ho_tried) return w->ho;
  w->ho_tried = true;
  const char* v = getenv("MACM_HANDOFF");
  if (!(v ? atoi(v) != 0 : kHandoffDefault) || serialized_dispatch()) return nullptr;
  HandoffStream* h = new HandoffStream{};
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&h->done, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&h->pre_b, hipEventDisableTiming) == hipSuccess &&
            hipMalloc(&h->b_started, sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc(&h->ctr, 2 * sizeof(unsigned int)) == hipSuccess &&
            hipMalloc(&h->q, (size_t)w->P.n_envs * sizeof(unsigned long long)) == hipSuccess;
  // tags start at 1, so a zeroed queue holds no entry of any step; the start count from 0
  ok = ok && hipMemset(h->q, 0, (size_t)w->P.n_envs * sizeof(unsigned long long)) == hipSuccess &&
       hipMemset(h->ctr, 0, 2 * sizeof(unsigned int)) == hipSuccess &&
       hipMemset(h->b_started, 0, sizeof(unsigned long long)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    free_handoff(h);
    return nullptr;
  }
  w->ho = h;
  return h;
}

// A call's I/O: the caller's actions and outputs, the world's obs type. step_outputs moves it to a
// trajectory's row, rollout_wg_slices to a slice's envs.
static FlockIO world_io(const macm_world* w, const void* actions, const macm_outputs& out) {
  FlockIO io;
  io.actions = actions;
  io.obs = out.obs;
  io.obs_f64 = w->cfg.obs_f64 != 0;
  io.nbr = out.nbr_id;
  io.rew = out.reward;
  io.coll = out.collided;
  io.done = out.done;
  return io;
}

int macm_world_step(macm_world* w, const void* actions, const macm_outputs* out, void* stream) {
  if (!w || !actions || !out || !out->reward) return fail(MACM_E_INVALID, "world/actions/out/reward is NULL");
  if (w->autoreset && !w->mt_valid) return fail(MACM_E_INVALID, kNoStreams);
  if (const int rc = final_outputs_need(w->autoreset, w->fin, out->obs, out->nbr_id, nullptr)) return rc;
  if (const uint32_t st = read_host_status(w->hstat)) return overflow_error(st);
  DeviceGuard g(w->device);
  if (w->cfg.validate_actions) {
    const int rc = check_actions(w->bad, actions, w->cfg.action_mode == MACM_ACTION_DISCRETE ? 0 : 1, nullptr,
                                 w->P.n_envs, w->P.n_agents, (hipStream_t)stream);
    if (rc) return rc;
  }
  const FlockIO io = world_io(w, actions, *out);
  if (w->wave)
    HIP_TRY(launch_step_w64(w->P, w->B, w->cur, io, (hipStream_t)stream));
  else if (w->big)
    HIP_TRY(launch_step_big(w->P, w->B, w->cur, io, (hipStream_t)stream));
  else
    HIP_TRY(launch_step_wg(w->P, w->B, w->cur, w->tcap, io, (hipStream_t)stream, handoff_for(w)));
  w->cur ^= 1;
  if (w->autoreset) return world_autoreset_step(w, out, (hipStream_t)stream);
  return MACM_OK;
}

// Envs [e0, e0 + n) of a world as a world of n envs: every per-env array offset by e0 rows
// (the sizes macm_world_create allocates), tidx and the status word shared.
static WorldBuffers slice_buffers(const WorldBuffers& B, size_t e0, size_t N, size_t T, size_t C, size_t tcap) {
  WorldBuffers S = B;
  const size_t EN = e0 * N, IS = e0 * (N / 2 + 2);
  auto off = [](auto*& p, size_t n) {
    if (p) p += n;
  };
  off(S.pos, EN), off(S.vel, EN), off(S.angle, EN), off(S.fat, EN), off(S.sleep, EN);
  off(S.targets, e0 * T);
  for (int c = 0; c < 2; ++c) off(S.ccount[c], e0), off(S.cab[c], e0 * C), off(S.cimp[c], e0 * C);
  off(S.step_count, e0), off(S.time_passed, e0), off(S.done, e0), off(S.status, e0);
  off(S.env_counters, e0 * 4), off(S.env_rsum, e0), off(S.stamps, e0 * 32);
  off(S.scratch, e0 * tcap), off(S.x_cst, e0 * tcap), off(S.x_cimp, e0 * tcap), off(S.x_ord, e0 * tcap);
  off(S.x_ic, IS), off(S.x_nlvl, e0), off(S.x_ib, IS), off(S.x_ibod, EN), off(S.x_nisl, e0);
  off(S.x_vmid, EN), off(S.x_cout, EN), off(S.x_vout, EN), off(S.x_deg, EN), off(S.x_isolv, IS);
  off(S.x_tab, e0 * tcap), off(S.x_adj, e0 * 2 * tcap), off(S.x_off, e0 * (N + 1)), off(S.x_dfs, e0 * tcap);
  off(S.spill_count, e0);
  off(S.sched, e0);  // a slice's order holds slice-local env ids (launch_env_order on the slice)
  if (B.sp_pool == 0) {  // one working-set slot per env: the slice's rows; a pool is shared as it is
    off(S.sp_tab, e0 * C), off(S.sp_adj, e0 * 2 * C), off(S.sp_ord, e0 * C), off(S.sp_cst, e0 * C);
    off(S.sp_cim, e0 * C), off(S.sp_lam, e0 * C);
    if (B.sp_rec) S.sp_rec = static_cast<float4*>(B.sp_rec) + EN * 3;  // 48-B records
  }
  return S;
}

// Step k's outputs: row k of [K, ...] buffers in the trajectory form (macm_world_rollout_traj),
// else the one set every step overwrites.
static macm_outputs step_outputs(const macm_world* w, const macm_outputs* out, int k, bool traj) {
  macm_outputs o = *out;
  if (!traj || k == 0) return o;
  const size_t E = w->P.n_envs, EN = E * w->P.n_agents;
  const size_t obytes = EN * obs_dim(w->cfg) * (w->cfg.obs_f64 ? sizeof(double) : sizeof(float));
  if (o.obs) o.obs = static_cast<unsigned char*>(o.obs) + k * obytes;
  if (o.nbr_id) o.nbr_id += k * EN;
  if (o.reward) o.reward += k * EN;
  if (o.collided) o.collided += k * EN;
  if (o.done) o.done += k * E;
  return o;
}

// Workgroup-path rollout over env slices on streams of their own. The step is three launches whose
// durations are each set by the slowest env, so the K steps of kSlices env slices run on their own
// streams with no join between steps: one slice's next kernels fill another's tails. Forked from
// and joined back into the caller's stream; results are those of the per-step launches (envs are
// independent). Measured at C3 (4096 x 256, steps 6-25): 568 -> 484 us per step with 2 slices,
// 481 with 3, but 744 with 4: with the caller's stream that is more streams than the process's 4
// hardware queues (GPU_MAX_HW_QUEUES), and two slices sharing a queue serialise each other's
// launches. C5 (N = 1024, 2048 envs) gained nothing (profiles/r02/rollout/).
static constexpr int kSlices = 3, kSliceMinEnvs = 1024, kSliceMaxAgents = 512;
// MACM_WG_SLICES=n: n env slices (0: none, the handoff instead; A/B sessions), kSlices by default
static int n_slices() {
  const char* v = getenv("MACM_WG_SLICES");
  const int n = v ? atoi(v) : kSlices;
  return n < 0 ? 0 : n > 8 ? 8 : n;
}
// the env slices a workgroup-path rollout of this world runs (0: none, one stream)
static int wg_rollout_slices(const macm_world* w) {
  if (w->wave || w->big || w->P.n_envs < kSliceMinEnvs || w->P.n_agents >= kSliceMaxAgents) return 0;
  if (w->autoreset) return 0;  // the reset launches follow each step's on the one stream (env slices: a follow-up)
  const int S = n_slices();
  return S >= 2 ? S : 0;
}
// astride == 0: the closed loop (macm_world_rollout_bots): every step of a slice reads the bot's
// action rows of its envs and the bots kernel writes the next ones from the slice's obs rows
// (trajectory form: step k reads action row k and writes row k + 1 of [K + 1, E, N, 3]).
static int rollout_wg_slices(macm_world* w, int S, const unsigned char* actions, int n_steps,
                             unsigned long long astride, const macm_outputs* out, bool traj, hipStream_t user) {
  const int E = w->P.n_envs, N = w->P.n_agents;
  if ((int)w->slice_streams.size() < S) {
    for (int i = (int)w->slice_streams.size(); i < S; ++i) {
      hipStream_t st;
      HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      w->slice_streams.push_back(st);
    }
  }
  while ((int)w->slice_events.size() < S + 1) {
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    w->slice_events.push_back(ev);
  }
  const size_t od = (size_t)N * obs_dim(w->cfg) * (w->cfg.obs_f64 ? sizeof(double) : sizeof(float));
  const bool bots = astride == 0;
  const size_t abytes = bots ? 3 * (size_t)N : astride / (size_t)E;
  const unsigned long long kstride = bots ? (traj ? (unsigned long long)E * abytes : 0ull) : astride;
  HIP_TRY(hipEventRecord(w->slice_events[0], user));
  std::vector<StepParams> Ps(S, w->P);
  std::vector<WorldBuffers> Bs(S);
  std::vector<size_t> e0s(S);
  for (int i = 0; i < S; ++i) {
    const size_t e0 = (size_t)E * i / S, e1 = (size_t)E * (i + 1) / S;
    e0s[i] = e0;
    Ps[i].n_envs = (int)(e1 - e0);
    Bs[i] = slice_buffers(w->B, e0, N, w->P.n_targets, w->P.max_contacts, w->tcap);
    HIP_TRY(hipStreamWaitEvent(w->slice_streams[i], w->slice_events[0], 0));
  }
  // every launch is enqueued before the join below; a failed launch still joins the slice streams
  // into the caller's (no unjoined work left behind) and leaves the list parity of
  // the steps that were launched
  int rc = MACM_OK, launched = 0;
  for (int k = 0; k < n_steps && rc == MACM_OK; ++k) {
    const int cur = w->cur ^ (k & 1);
    const macm_outputs ok = step_outputs(w, out, k, traj);
    for (int i = 0; i < S && rc == MACM_OK; ++i) {
      const size_t e0 = e0s[i];
      auto row = [e0](auto* p, size_t per_env) { return p ? p + e0 * per_env : p; };
      unsigned char* obs_i = ok.obs ? static_cast<unsigned char*>(ok.obs) + e0 * od : nullptr;
      const unsigned char* act_k = actions + k * kstride + e0 * abytes;
      // closed loop: kernel C takes the bot's next actions from the rows it writes (no bots launch)
      uint8_t* const bot = bots ? const_cast<unsigned char*>(act_k) + (traj ? (size_t)E * abytes : 0) : nullptr;
      FlockIO io = world_io(w, act_k, ok);  // the slice's rows of step k's
      io.obs = obs_i;
      io.nbr = row(ok.nbr_id, N);
      io.rew = row(ok.reward, N);
      io.coll = row(ok.collided, N);
      io.done = row(ok.done, 1);
      const hipError_t he = launch_step_wg(Ps[i], Bs[i], cur, w->tcap, io, w->slice_streams[i], nullptr, bot);
      if (he != hipSuccess) rc = fail(MACM_E_HIP, std::string("rollout launch: ") + hipGetErrorString(he));
    }
    if (rc == MACM_OK) ++launched;
  }
  for (int i = 0; i < S; ++i) {
    HIP_TRY(hipEventRecord(w->slice_events[1 + i], w->slice_streams[i]));
    HIP_TRY(hipStreamWaitEvent(user, w->slice_events[1 + i], 0));
  }
  if (launched & 1) w->cur ^= 1;
  return rc;
}

// macm_world_rollout / _traj (bots = false) and macm_world_rollout_bots / _traj (bots = true);
// macm_world_rollout_policy / _traj: the closed loop of bots = true with the registered policy as the
// actor (pol: its params and this call's noise and logits; NULL: the scripted bot);
// macm_world_rollout_policy_value / _traj: that with the registered critic beside the actor (crit: its
// params and this call's values and boot; NULL: none); smp: the policy draws its noise itself, the
// decision after step k at smp->decision + k (a world with sampling on; NULL: pol->noise)
static int world_rollout(macm_world* w, const void* actions, int n_steps, const macm_outputs* out, void* stream,
                         bool bots, bool traj, const PolicyArgs* pol = nullptr, const ValueArgs* crit = nullptr,
                         const SampleArgs* smp = nullptr) {
  if (n_steps < 0) return fail(MACM_E_INVALID, "n_steps must be >= 0");
  if (n_steps == 0) return MACM_OK;  // nothing is read, so actions may be NULL (an empty tensor)
  if (!w || !actions || !out || !out->reward) return fail(MACM_E_INVALID, "world/actions/out/reward is NULL");
  if (bots && !out->obs)
    return fail(MACM_E_INVALID, pol ? "out->obs is NULL (the policy acts on it)" : "out->obs is NULL (the bots act on it)");
  if (bots && w->cfg.action_mode != MACM_ACTION_DISCRETE) return fail(MACM_E_INVALID, "bots.flock acts in discrete mode");
  if (w->autoreset && !w->mt_valid) return fail(MACM_E_INVALID, kNoStreams);
  if (const int rc = final_outputs_need(w->autoreset, w->fin, out->obs, out->nbr_id, nullptr)) return rc;
  if (const uint32_t st = read_host_status(w->hstat)) return overflow_error(st);
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  const int mode = w->cfg.action_mode == MACM_ACTION_DISCRETE ? 0 : 1;
  if (w->cfg.validate_actions) {  // every step's actions before any env is stepped (bots: the caller's first)
    const long long rows = (long long)(bots ? 1 : n_steps) * w->P.n_envs;
    if (rows > INT32_MAX) return fail(MACM_E_INVALID, "n_steps * n_envs too large to validate");
    const int rc = check_actions(w->bad, actions, mode, nullptr, (int)rows, w->P.n_agents, s, w->P.n_envs);
    if (rc) return rc;
  }
  const unsigned long long astride =
      bots ? 0ull
           : (unsigned long long)w->P.n_envs * w->P.n_agents * (mode == 0 ? 3 * sizeof(uint8_t) : 2 * sizeof(float));
  if (w->wave) {  // one launch; astride 0: the closed-loop form of the rollout kernel
    const FlockIO io = world_io(w, actions, *out);
    const RollShape sh(n_steps, astride, traj);
    FlockRollExtras x;
    x.debug = w->roll_reload;
    x.policy = pol;
    x.critic = crit;
    x.sample = smp;
    if (w->autoreset)  // the kernels with the in-launch reset
      HIP_TRY(launch_rollout_ar_w64(w->P, w->B, w->cur, io, sh, x, ResetLaunch(w->mt, world_pose_draw(w), w->fin), s));
    else
      HIP_TRY(launch_rollout_w64(w->P, w->B, w->cur, io, sh, x, s));
    if (n_steps & 1) w->cur ^= 1;
    return MACM_OK;
  }
  const unsigned char* act = static_cast<const unsigned char*>(actions);
  if (!pol)  // (the policy loop: one stream, no env slices)
    if (const int S = wg_rollout_slices(w)) return rollout_wg_slices(w, S, act, n_steps, astride, out, traj, s);
  // workgroup path: its three launches per step (and the bot's), in order
  const long long rows = (long long)w->P.n_envs * w->P.n_agents;
  const unsigned long long kstride = bots ? (traj ? (unsigned long long)rows * 3 : 0ull) : astride;
  for (int k = 0; k < n_steps; ++k) {
    const macm_outputs ok = step_outputs(w, out, k, traj);
    const unsigned char* act_k = act + k * kstride;
    const FlockIO io = world_io(w, act_k, ok);
    if (w->big)
      HIP_TRY(launch_step_big(w->P, w->B, w->cur, io, s));
    else
      HIP_TRY(launch_step_wg(w->P, w->B, w->cur, w->tcap, io, s, handoff_for(w),
                             bots && !pol ? const_cast<unsigned char*>(act_k) + (traj ? rows * 3 : 0) : nullptr));
    w->cur ^= 1;
    // the critic: the bootstrap value from the obs the step produced, before any reset; the value of the
    // row the next action is taken from after it (without autoreset the same number: a device copy)
    float* const boot_k = crit && crit->boot ? crit->boot + (traj ? (size_t)k * rows : 0) : nullptr;
    float* const val_k = crit && crit->values ? crit->values + (traj ? (size_t)(k + 1) * rows : 0) : nullptr;
    if (crit) {
      float* const first = w->autoreset || boot_k ? boot_k : val_k;
      if (first) HIP_TRY(launch_value_flock(*crit, ok.obs, w->cfg.obs_f64 != 0, obs_dim(w->cfg), rows, first, s));
      if (!w->autoreset && boot_k && val_k)
        HIP_TRY(hipMemcpyAsync(val_k, boot_k, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (w->autoreset) {
      const int rc = world_autoreset_step(w, &ok, s);
      if (rc) return rc;
      if (val_k) HIP_TRY(launch_value_flock(*crit, ok.obs, w->cfg.obs_f64 != 0, obs_dim(w->cfg), rows, val_k, s));
    }
    // autoreset: kernel C's fused bot acted on the terminal observation; the bots launch over every
    // row takes a reset env's next actions from its new initial obs (the other rows: the same actions)
    if (bots && !pol && (w->big || w->autoreset))
      HIP_TRY(launch_bots_flock(ok.obs, w->cfg.obs_f64 != 0, obs_dim(w->cfg), rows,
                                const_cast<unsigned char*>(act_k) + (traj ? rows * 3 : 0), s));
    if (pol) {  // the policy over every row: noise row k, the logits into the step's output row
      PolicyArgs M = *pol;
      if (M.noise) M.noise += (size_t)k * rows * kPolicyLogits;
      if (M.logits && traj) M.logits += (size_t)k * rows * kPolicyLogits;
      unsigned char* const next = const_cast<unsigned char*>(act_k) + (traj ? rows * 3 : 0);
      if (smp)  // the same draws as the wave path's launch
        HIP_TRY(launch_policy_flock_sampled(M, SampleArgs{smp->seed, smp->decision + (unsigned long long)k, smp->row0},
                                            ok.obs, w->cfg.obs_f64 != 0, obs_dim(w->cfg), rows, next, s));
      else
        HIP_TRY(launch_policy_flock(M, ok.obs, w->cfg.obs_f64 != 0, obs_dim(w->cfg), rows, next, s));
    }
  }
  return MACM_OK;
}

int macm_world_rollout(macm_world* w, const void* actions, int n_steps, const macm_outputs* out, void* stream) {
  return world_rollout(w, actions, n_steps, out, stream, false, false);
}

int macm_world_rollout_traj(macm_world* w, const void* actions, int n_steps, const macm_outputs* traj,
                            void* stream) {
  return world_rollout(w, actions, n_steps, traj, stream, false, true);
}

int macm_world_rollout_bots(macm_world* w, uint8_t* actions, int n_steps, const macm_outputs* out, void* stream) {
  return world_rollout(w, actions, n_steps, out, stream, true, false);
}

int macm_world_rollout_bots_traj(macm_world* w, uint8_t* actions, int n_steps, const macm_outputs* traj,
                                 void* stream) {
  return world_rollout(w, actions, n_steps, traj, stream, true, true);
}

// macm_world_set_policy / _set_critic: the caller's struct into the world's slot (NULL: cleared)
extern "C++" template <typename M>
static int world_set_mlp(macm_world* w, const std::string& noun, const char* discrete_only, const M* m, M* slot) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  if (!m) {
    *slot = M{0, 0, 0, 0, nullptr};
    return MACM_OK;
  }
  if (const int rc = mlp_check(noun, m)) return rc;
  if (w->cfg.action_mode != MACM_ACTION_DISCRETE) return fail(MACM_E_UNSUPPORTED, noun + discrete_only);
  if (m->in_dim != obs_dim(w->cfg))
    return fail(MACM_E_INVALID, noun + ": in_dim " + std::to_string(m->in_dim) + " is not the world's obs_dim " +
                                    std::to_string(obs_dim(w->cfg)));
  *slot = *m;
  return MACM_OK;
}

int macm_world_set_policy(macm_world* w, const macm_policy_mlp* p) {
  return world_set_mlp(w, "policy", ": the MLP policy acts in discrete mode (MultiDiscrete([3, 3, 3]))", p,
                       w ? &w->policy : nullptr);
}

// macm_world_set_sampling / _at / _get_sampling / _get_sampling_row: the draw as a property of the world
// (cfg NULL: off); first_row: the job's row of the world's row 0 (a shard's env_offset * n_agents)
int macm_world_set_sampling_at(macm_world* w, const macm_sample_config* cfg, int64_t first_row) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  if (!cfg) {
    w->sampling = false;
    w->sample = SampleArgs{0, 0, 0};
    return MACM_OK;
  }
  if (const int rc = sample_check(cfg, (int64_t)w->P.n_envs * w->P.n_agents, first_row)) return rc;
  if (w->cfg.action_mode != MACM_ACTION_DISCRETE)
    return fail(MACM_E_UNSUPPORTED, "sampling: the MLP policy acts in discrete mode (MultiDiscrete([3, 3, 3]))");
  w->sampling = true;
  w->sample = SampleArgs{cfg->seed, cfg->decision, (uint32_t)first_row};
  return MACM_OK;
}

int macm_world_set_sampling(macm_world* w, const macm_sample_config* cfg) {
  return macm_world_set_sampling_at(w, cfg, 0);
}

int macm_world_get_sampling_row(macm_world* w, int64_t* first_row) {
  if (!w || !first_row) return fail(MACM_E_INVALID, "world/first_row is NULL");
  *first_row = (int64_t)w->sample.row0;  // exact: a world has rows, so first_row < 2^32 was required
  return w->sampling ? 1 : 0;
}

int macm_world_get_sampling(macm_world* w, macm_sample_config* cfg_out) {
  if (!w || !cfg_out) return fail(MACM_E_INVALID, "world/cfg_out is NULL");
  *cfg_out = macm_sample_config{w->sample.seed, w->sample.decision, {0, 0, 0, 0}};
  return w->sampling ? 1 : 0;
}

static const char* const kNoiseAndSampling =
    "noise is given while sampling is on (macm_world_set_sampling): the launch draws its own; nothing was launched";
// the draw of a policy rollout of w (NULL: sampling is off)
static const SampleArgs* world_sample(const macm_world* w) { return w->sampling ? &w->sample : nullptr; }

static int world_rollout_policy(macm_world* w, uint8_t* actions, int n_steps, const float* noise, float* logits,
                                const macm_outputs* out, void* stream, bool traj) {
  if (n_steps < 0) return fail(MACM_E_INVALID, "n_steps must be >= 0");
  if (n_steps == 0) return MACM_OK;
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  if (!w->policy.params) return fail(MACM_E_INVALID, "no policy is registered (macm_world_set_policy)");
  if (w->sampling && noise) return fail(MACM_E_INVALID, kNoiseAndSampling);
  const PolicyArgs M{w->policy.params, noise, logits, w->policy.hidden, w->policy.n_hidden};
  const int rc = world_rollout(w, actions, n_steps, out, stream, true, traj, &M, nullptr, world_sample(w));
  if (rc == MACM_OK && w->sampling) w->sample.decision += (unsigned long long)n_steps;
  return rc;
}

int macm_world_rollout_policy(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                              const macm_outputs* out, void* stream) {
  return world_rollout_policy(w, actions, n_steps, noise, logits, out, stream, false);
}

int macm_world_rollout_policy_traj(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                                   const macm_outputs* traj, void* stream) {
  return world_rollout_policy(w, actions, n_steps, noise, logits, traj, stream, true);
}

int macm_world_set_critic(macm_world* w, const macm_value_mlp* c) {
  return world_set_mlp(w, "critic", ": it runs beside the MLP policy, which acts in discrete mode", c,
                       w ? &w->critic : nullptr);
}

static int world_rollout_policy_value(macm_world* w, uint8_t* actions, int n_steps, const float* noise, float* logits,
                                      float* values, float* boot, const macm_outputs* out, void* stream, bool traj) {
  if (n_steps < 0) return fail(MACM_E_INVALID, "n_steps must be >= 0");
  if (n_steps == 0) return MACM_OK;
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  if (!values && !boot)
    return fail(MACM_E_INVALID, "values and boot are both NULL (macm_world_rollout_policy serves that case)");
  if (!w->policy.params) return fail(MACM_E_INVALID, "no policy is registered (macm_world_set_policy)");
  if (!w->critic.params) return fail(MACM_E_INVALID, "no critic is registered (macm_world_set_critic)");
  if (w->sampling && noise) return fail(MACM_E_INVALID, kNoiseAndSampling);
  const PolicyArgs M{w->policy.params, noise, logits, w->policy.hidden, w->policy.n_hidden};
  const ValueArgs V{w->critic.params, values, boot, w->critic.hidden, w->critic.n_hidden};
  const int rc = world_rollout(w, actions, n_steps, out, stream, true, traj, &M, &V, world_sample(w));
  if (rc == MACM_OK && w->sampling) w->sample.decision += (unsigned long long)n_steps;
  return rc;
}

int macm_world_rollout_policy_value(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                                    float* values, float* boot, const macm_outputs* out, void* stream) {
  return world_rollout_policy_value(w, actions, n_steps, noise, logits, values, boot, out, stream, false);
}

int macm_world_rollout_policy_value_traj(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise,
                                         float* logits, float* values, float* boot, const macm_outputs* traj,
                                         void* stream) {
  return world_rollout_policy_value(w, actions, n_steps, noise, logits, values, boot, traj, stream, true);
}

int macm_world_observe(macm_world* w, const macm_outputs* out, void* stream) {
  if (!w || !out) return fail(MACM_E_INVALID, "world/out is NULL");
  DeviceGuard g(w->device);
  if (w->wave)
    HIP_TRY(launch_observe_w64(w->P, w->B, out->obs, w->cfg.obs_f64 != 0, out->nbr_id, (hipStream_t)stream));
  else if (w->big)
    HIP_TRY(launch_observe_big(w->P, w->B, out->obs, w->cfg.obs_f64 != 0, out->nbr_id, (hipStream_t)stream));
  else
    HIP_TRY(launch_observe_wg(w->P, w->B, out->obs, w->cfg.obs_f64 != 0, out->nbr_id, (hipStream_t)stream));
  return MACM_OK;
}

static int copy_state(macm_world* w, const macm_state* st, void* stream, bool to_device) {
  if (!w || !st) return fail(MACM_E_INVALID, "world/state is NULL");
  if (st->contact_stride < 0) return fail(MACM_E_INVALID, "contact_stride must be >= 0");
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t E = w->P.n_envs, N = w->P.n_agents, T = w->P.n_targets;
  if (const int rc = copy_state_lists(w, st, to_device, s)) return rc;
  struct Item {
    void* user;
    void* dev;
    size_t bytes;
  } items[] = {
      {st->pos, w->B.pos, E * N * sizeof(float2)},
      {st->vel, w->B.vel, E * N * sizeof(float2)},
      {st->angle, w->B.angle, E * N * sizeof(float)},
      {st->fat, w->B.fat, E * N * sizeof(float4)},
      {st->sleep, w->B.sleep, E * N * sizeof(float)},
      {st->targets, w->B.targets, E * T * sizeof(float2)},
      {st->step_count, w->B.step_count, E * sizeof(int32_t)},
      {st->time_passed, w->B.time_passed, E * sizeof(double)},
  };
  for (const Item& it : items) {
    if (!it.user) continue;
    if (to_device) HIP_TRY(hipMemcpyAsync(it.dev, it.user, it.bytes, hipMemcpyDefault, s));
    else HIP_TRY(hipMemcpyAsync(it.user, it.dev, it.bytes, hipMemcpyDefault, s));
  }
  if (to_device && st->time_passed) {
    // done flag follows time_passed (mvmnt.py:135-136)
    std::vector<double> tp(E);
    std::vector<uint8_t> dn(E);
    HIP_TRY(hipMemcpyAsync(tp.data(), w->B.time_passed, E * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t e = 0; e < E; ++e) dn[e] = tp[e] > w->P.time_limit ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(w->B.done, dn.data(), E, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return MACM_OK;
}

int macm_world_get_state(macm_world* w, const macm_state* dst, void* stream) {
  return copy_state(w, dst, stream, false);
}

int macm_world_set_state(macm_world* w, const macm_state* src, void* stream) {
  return copy_state(w, src, stream, true);
}

int macm_world_status(macm_world* w, int32_t* status_or, void* stream) { return world_status(w, status_or, stream); }

int macm_world_counters(macm_world* w, int64_t out[4], void* stream) { return world_counters(w, out, stream); }

int macm_world_reset_counters(macm_world* w, void* stream) {
  if (!w) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  HIP_TRY(hipMemsetAsync(w->B.env_counters, 0, (size_t)w->P.n_envs * 4 * sizeof(unsigned long long),
                         (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(w->B.env_rsum, 0, (size_t)w->P.n_envs * sizeof(double), (hipStream_t)stream));
  return MACM_OK;
}

// Per-env reward sums (flock_common.hpp: each step's float32 rewards as float64, pairwise over the
// agent slots, added to the env's total in step order) and their sum over envs in env order, starting
// from +0.0: a fixed order throughout, so the total is bit-stable for any launch form or env slicing.
// Binary rewards are -1, 0 or +1, so every partial sum in that order is an exact integer and an env's
// total is exactly (positive-reward agent-steps) - (collided agent-steps), its counters 2 and 1: the
// kernels accumulate env_rsum for linear rewards only (a binary world's per-step sum and atomic add
// cost 2.5% of the steady-state step, profiles/r06/abtests/rsum/).
int macm_world_reward_sums(macm_world* w, double* per_env, double* total, void* stream) {
  if (!w || (!per_env && !total)) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  std::vector<double> h((size_t)w->P.n_envs);
  hipStream_t s = (hipStream_t)stream;
  if (w->P.reward_mode == MACM_REWARD_LINEAR) {
    HIP_TRY(hipMemcpyAsync(h.data(), w->B.env_rsum, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else {
    std::vector<unsigned long long> c(h.size() * 4);
    HIP_TRY(hipMemcpyAsync(c.data(), w->B.env_counters, c.size() * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t e = 0; e < h.size(); ++e) h[e] = (double)((long long)c[e * 4 + 2] - (long long)c[e * 4 + 1]);
  }
  if (per_env) memcpy(per_env, h.data(), h.size() * sizeof(double));
  if (total) {
    double acc = 0.0;
    for (double v : h) acc += v;
    *total = acc;
  }
  return MACM_OK;
}

int macm_world_spilled(macm_world* w, int64_t* env_steps, void* stream) {
  return world_spilled(w, env_steps, stream);
}

int macm_world_set_debug(macm_world* w, int32_t flags) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  const int pool = (flags & MACM_DEBUG_SPILL_POOL) ? (flags >> 8) : 0;
  flags &= 0xff;
  if (flags & ~(MACM_DEBUG_FORCE_SPILL | MACM_DEBUG_SWEEP_CELLS | MACM_DEBUG_SWEEP_ALL_PAIRS | MACM_DEBUG_SPILL_POOL | MACM_DEBUG_SPILL_FAIL |
                MACM_DEBUG_ROLLOUT_RELOAD | MACM_DEBUG_NEAR_PLAIN))
    return fail(MACM_E_INVALID, "unknown debug flag");
  if ((flags & MACM_DEBUG_SWEEP_CELLS) && (flags & MACM_DEBUG_SWEEP_ALL_PAIRS))
    return fail(MACM_E_INVALID, "SWEEP_CELLS and SWEEP_ALL_PAIRS exclude each other");
  if (int rc = set_spill_pool(w, flags, pool)) return rc;
  w->P.force_spill = (flags & MACM_DEBUG_FORCE_SPILL) ? 1 : 0;
  w->roll_reload = ((flags & MACM_DEBUG_ROLLOUT_RELOAD) ? 1 : 0) | ((flags & MACM_DEBUG_NEAR_PLAIN) ? 2 : 0);
  w->P.sweep = (flags & MACM_DEBUG_SWEEP_CELLS) ? 1 : (flags & MACM_DEBUG_SWEEP_ALL_PAIRS) ? 2 : 0;
  return MACM_OK;
}

#ifdef MACM_STAMPS
// Diagnostic build only: copy the per-env phase stamps [E, 32] of the last step (the wave kernel
// uses rows of 16).
int macm_debug_stamps(macm_world* w, unsigned long long* out) {
  if (!w || !out) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  HIP_TRY(hipMemcpy(out, w->B.stamps, (size_t)w->P.n_envs * 32 * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost));
  return MACM_OK;
}
#endif

}  // extern "C"
