// capi_tdm.hip — the TDM worlds of the C-ABI of libmacm_hip.so (declared in include/macm.h).
//
// Owns the per-world device state (SoA, sized for E envs x N agents), derives the step constants from
// macm_tdm_config the way the reference derives them, seeds envs with the reference's RNG order, and
// launches the HIP kernels on the caller's stream. No torch types, no exceptions across the ABI.
#include "capi_common.hpp"

struct macm_tdm {
  macm_tdm_config cfg;
  StepParams P;
  WorldBuffers B;
  TdmParams TP;
  TdmBuffers TB;  // state pointers; output pointers are filled per call
  int cur;
  int device;
  bool wave;  // N <= 64: the wave kernel (env_step_w64<kTdm>); else the workgroup step (tdm_step_wg.hip)
  std::vector<int> team;  // agent -> team
  std::vector<void*> allocs;
  uint32_t* mt = nullptr;
  uint8_t* rmask = nullptr;
  bool mt_valid = false;
  bool autoreset = false;  // macm_tdm_set_autoreset
  FinalOut fin{};          // macm_tdm_set_final_outputs
  // macm_tdm_set_events: the caller's buffer, kept until replaced or cleared (hit_id NULL: none; the
  // steps then launch the kernels without events, the ones they have always launched)
  macm_tdm_events events{nullptr, 0};
  // macm_tdm_set_policy: the caller's struct (params NULL: none), the teams it acts for, and their agents
  // as the one-shot kernel's [N] mask on the device (the workgroup path's per-step loop; NULL: every team)
  macm_tdm_policy policy{0, {0, 0, 0}, nullptr};
  uint32_t policy_teams = 0;
  uint8_t* policy_agents = nullptr;
  bool policy_all = false;
  uint32_t* hstat = nullptr;
  unsigned long long* bad = nullptr;
  int slots_alloc = 0;  // as macm_world
  int pool0 = 0;
  // the split observation (tdm_obs_snap.hip, tdm_split_obs): pose snapshots in two halves of
  // snap_rows (step, env) rows each, the observation stream and the chunk events (created on first use)
  float4* snap = nullptr;
  size_t snap_rows = 0;
  hipStream_t obs_stream = nullptr;
  hipEvent_t ev_phys[2] = {nullptr, nullptr}, ev_obs[2] = {nullptr, nullptr};
  // the tail observation (flock_step_w64.hip TailObs, tdm_tail_obs): snapshots of every (step, env)
  // row of a rollout, the row counters and ready words, the last launch's tag, the resident capacity
  float4* tail_snap = nullptr;
  size_t tail_rows = 0;
  unsigned long long* tail_ctl = nullptr;
  unsigned tail_tag = 0;
  int tail_cap = -1;
};

extern "C" {

int macm_tdm_config_default(macm_tdm_config* c) {
  if (!c) return fail(MACM_E_INVALID, "cfg is NULL");
  memset(c, 0, sizeof(*c));
  c->n_teams = 2;  // TDM(n_agents=[1, 1]) default, combat.py:62
  c->team_size[0] = 1;
  c->team_size[1] = 1;
  c->n_agents = 2;
  c->velocity_iterations = 8;
  c->position_iterations = 3;
  c->warm_starting = 1;
  c->obs_f64 = 0;
  c->fresh_raycast = 0;
  c->decay_mov_penalty = 0;
  c->hz = 60.0;
  c->world_width = 30.0;
  c->world_height = 30.0;
  c->agent_rotation_speed = 0.8 * (2 * M_PI);
  c->agent_force = 20.0;
  c->percent_mov_penalty = 0.2;
  c->melee_range = 2.0;
  c->melee_dmg = 0.25;
  c->init_health = 1.0;
  c->cooldown_atk = 1.0;
  c->cooldown_mov_penalty = 0.5;
  c->time_limit = 60.0;
  c->radius = 0.5f;
  c->density = 1.0f;
  c->friction = 0.3f;
  c->linear_damping = 5.0f;
  return MACM_OK;
}

static void free_tdm(macm_tdm* w) {
  for (void* p : w->allocs) (void)hipFree(p);
  w->allocs.clear();
  if (w->snap) (void)hipFree(w->snap);
  w->snap = nullptr;
  if (w->tail_snap) (void)hipFree(w->tail_snap);
  w->tail_snap = nullptr;
  if (w->tail_ctl) (void)hipFree(w->tail_ctl);
  w->tail_ctl = nullptr;
  if (w->obs_stream) (void)hipStreamDestroy(w->obs_stream);
  w->obs_stream = nullptr;
  for (int b = 0; b < 2; ++b) {
    if (w->ev_phys[b]) (void)hipEventDestroy(w->ev_phys[b]);
    if (w->ev_obs[b]) (void)hipEventDestroy(w->ev_obs[b]);
    w->ev_phys[b] = w->ev_obs[b] = nullptr;
  }
  if (w->hstat) (void)hipHostFree(w->hstat);
  w->hstat = nullptr;
}

int macm_tdm_create(const macm_tdm_config* cfg, int32_t n_envs, int32_t device, macm_tdm** out) {
  if (!cfg || !out) return fail(MACM_E_INVALID, "cfg/out is NULL");
  *out = nullptr;
  const macm_tdm_config& c = *cfg;
  if (n_envs <= 0) return fail(MACM_E_INVALID, "n_envs must be > 0");
  if (c.n_teams < 1 || c.n_teams > 4) return fail(MACM_E_INVALID, "n_teams must be in [1, 4]");
  int N = 0;
  for (int t = 0; t < c.n_teams; ++t) {
    if (c.team_size[t] < 0) return fail(MACM_E_INVALID, "team_size < 0");
    N += c.team_size[t];
  }
  if (N != c.n_agents) return fail(MACM_E_INVALID, "n_agents != sum(team_size)");
  if (N < 2) return fail(MACM_E_INVALID, "n_agents must be >= 2");
  // N > 64: the workgroup step (tdm_step_wg.hip), one thread per agent and 16-bit body ids in the
  // contact list, as the Flock workgroup path
  if (N > kMaxAgents) return fail(MACM_E_UNSUPPORTED, "TDM with more than 4096 agents per env is not built");
  if (!(c.hz > 0.0)) return fail(MACM_E_INVALID, "hz must be > 0");
  if (c.velocity_iterations < 0 || c.position_iterations < 0) return fail(MACM_E_INVALID, "iterations < 0");
  if (!(c.radius > 0.0f)) return fail(MACM_E_INVALID, "radius must be > 0");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MACM_E_INVALID, "device index out of range");
  DeviceGuard g(device);
  size_t free_bytes = 0, total_bytes = 0;
  HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
  if (N > 64) {
    int max_lds = 0;
    HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    const int need = std::max(tdm_wg_step_lds(N), tdm_wg_obs_lds(N));
    if (need > max_lds)
      return fail(MACM_E_UNSUPPORTED, "TDM workgroup step needs " + std::to_string(need) + " B of LDS, device has " +
                                          std::to_string(max_lds));
    HIP_TRY(tdm_wg_configure(N));
  }

  macm_tdm* w = new macm_tdm();
  w->cfg = c;
  w->device = device;
  w->cur = 0;
  w->wave = N <= 64;
  const int C = N * (N - 1) / 2;  // every pair: the list never overflows
  // spill working-set slots from the device budget, as Flock's: one per env when they fit, else a
  // pool. Both TDM callers take their slot before committing anything of the step (the wave
  // kernel's hand-over and the workgroup step), so a pool wait leaves an env wholly unstepped,
  // never half-stepped (N <= 64 used to take one slot per env regardless of memory)
  const int64_t SL = default_capacity(N, n_envs, C, free_bytes).slots;
  StepParams& P = w->P;
  memset(&P, 0, sizeof(P));
  P.n_envs = n_envs;
  P.n_agents = N;
  P.n_targets = 0;
  P.max_contacts = C;
  P.vel_iters = c.velocity_iterations;
  P.pos_iters = c.position_iterations;
  P.warm_starting = c.warm_starting ? 1 : 0;
  P.action_mode = MACM_ACTION_DISCRETE;
  P.reward_mode = MACM_REWARD_BINARY;
  P.coord = MACM_COORD_POLAR;
  fill_body_params(P, c.hz, c.radius, c.density, c.friction, c.linear_damping, c.agent_force,
                   c.agent_rotation_speed);
  P.time_limit = c.time_limit;
  TdmParams& TP = w->TP;
  memset(&TP, 0, sizeof(TP));
  TP.n_teams = c.n_teams;
  for (int t = 0, acc = 0; t < 4; ++t) {
    acc += t < c.n_teams ? c.team_size[t] : 0;
    TP.team_end[t] = acc;
  }
  TP.fresh_raycast = c.fresh_raycast ? 1 : 0;
  TP.decay_mov_penalty = c.decay_mov_penalty ? 1 : 0;
  TP.melee_range = c.melee_range;
  TP.melee_dmg = c.melee_dmg;
  TP.cooldown_atk = c.cooldown_atk;
  TP.cooldown_mov_penalty = c.cooldown_mov_penalty;
  TP.percent_mov_penalty = c.percent_mov_penalty;
  TP.init_health = c.init_health;
  w->team.resize(N);
  for (int i = 0; i < N; ++i) w->team[i] = tdm_team_of(TP, i);

  WorldBuffers& B = w->B;
  TdmBuffers& TB = w->TB;
  memset(&B, 0, sizeof(B));
  memset(&TB, 0, sizeof(TB));
  const size_t EN = (size_t)n_envs * N, E = (size_t)n_envs;
  std::vector<void*>& A = w->allocs;
  int rc = MACM_OK;
  if ((rc = dalloc(A, &B.pos, EN)) || (rc = dalloc(A, &B.vel, EN)) || (rc = dalloc(A, &B.angle, EN)) ||
      (rc = dalloc(A, &B.fat, EN)) || (rc = dalloc(A, &B.sleep, EN)) || (rc = dalloc(A, &B.ccount[0], E)) ||
      (rc = dalloc(A, &B.ccount[1], E)) || (rc = dalloc(A, &B.cab[0], E * C)) ||
      (rc = dalloc(A, &B.cab[1], E * C)) || (rc = dalloc(A, &B.cimp[0], E * C)) ||
      (rc = dalloc(A, &B.cimp[1], E * C)) || (rc = dalloc(A, &B.step_count, E)) ||
      (rc = dalloc(A, &B.time_passed, E)) || (rc = dalloc(A, &B.done, E)) || (rc = dalloc(A, &B.status, E)) ||
      (rc = dalloc(A, &B.env_counters, E * 4)) || (rc = dalloc(A, &TB.health, EN)) ||
      (rc = dalloc(A, &TB.cd_atk, EN)) || (rc = dalloc(A, &TB.cd_mov, EN)) || (rc = dalloc(A, &TB.alive, EN)) ||
      (rc = dalloc(A, &TB.listener, E)) || (rc = dalloc(A, &TB.winner, E)) || (rc = dalloc(A, &w->bad, 1)) ||
      (rc = dalloc(A, &w->mt, E * kMtStride)) || (rc = dalloc(A, &w->rmask, E)) ||
      // the spill step's working set (an env with more than 256 touching contacts or 16 per body):
      // C = every pair; its body records in HBM too (the TDM kernel's LDS pool holds the rest)
      (rc = dalloc(A, &B.sp_tab, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_adj, (size_t)SL * 2 * C)) ||
      (rc = dalloc(A, &B.sp_ord, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_cst, (size_t)SL * C)) ||
      (rc = dalloc(A, &B.sp_cim, (size_t)SL * C)) || (rc = dalloc(A, &B.sp_lam, (size_t)SL * C)) ||
      (rc = dalloc(A, (float4**)&B.sp_rec, (size_t)SL * N * 3)) ||  // 48-B records
      (SL < n_envs && (rc = dalloc(A, &B.sp_lock, (size_t)SL))) || (rc = dalloc(A, &B.spill_count, E)) ||
      (w->wave && (rc = dalloc(A, &B.sched, (size_t)E)))
#ifdef MACM_STAMPS
      || (rc = dalloc(A, &B.stamps, E * 32))
#endif
  ) {
    free_tdm(w);
    delete w;
    return rc;
  }
  if (hipError_t he = alloc_host_status(&w->hstat, &B.host_status); he != hipSuccess) {
    free_tdm(w);
    delete w;
    return fail(MACM_E_OOM, std::string("hipHostMalloc (status word): ") + hipGetErrorString(he));
  }
  hipError_t e = hipMemset(B.env_counters, 0, E * 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(B.ccount[0], 0, sizeof(int32_t) * E);
  if (e == hipSuccess) e = hipMemset(B.status, 0, sizeof(int32_t) * E);
  if (e == hipSuccess) e = hipMemset(B.spill_count, 0, sizeof(uint32_t) * E);
  B.sp_pool = SL < n_envs ? (int32_t)SL : 0;
  w->slots_alloc = (int)SL;
  w->pool0 = B.sp_pool;
  if (e == hipSuccess && B.sp_lock) e = hipMemset(B.sp_lock, 0, sizeof(uint32_t) * SL);
  if (e != hipSuccess) {
    free_tdm(w);
    delete w;
    return fail(MACM_E_HIP, std::string("tdm init: ") + hipGetErrorString(e));
  }
  *out = w;
  return MACM_OK;
}

int macm_tdm_destroy(macm_tdm* w) {
  if (!w) return MACM_OK;
  DeviceGuard g(w->device);
  (void)hipDeviceSynchronize();
  free_tdm(w);
  delete w;
  return MACM_OK;
}

static TdmBuffers tdm_with_outputs(const macm_tdm* w, const macm_tdm_outputs* out) {
  TdmBuffers TB = w->TB;
  if (out) {
    TB.mask_out = out->mask;
    TB.health_out = out->health;
    TB.alive_out = out->alive;
    TB.winner_out = out->winner;
  }
  return TB;
}

static hipError_t tdm_launch_init(const macm_tdm* w, const TdmBuffers& TB, void* obs, const uint8_t* mask,
                                  hipStream_t s) {
  if (w->wave) return launch_tdm_init_w64(w->P, w->B, w->TP, TB, w->cur, obs, w->cfg.obs_f64 != 0, mask, s);
  return launch_tdm_init_wg(w->P, w->B, w->TP, TB, w->cur, obs, w->cfg.obs_f64 != 0, mask, s);
}

// A call's I/O: the caller's actions, obs and done, the world's obs type and the first row of the
// registered events (macm_tdm_set_events; NULL: none). The callers move it on per step or chunk.
static TdmIO tdm_io(const macm_tdm* w, const void* actions, const macm_tdm_outputs* out) {
  TdmIO io;
  io.actions = actions;
  io.obs = out ? out->obs : nullptr;
  io.obs_f64 = w->cfg.obs_f64 != 0;
  io.done = out ? out->done : nullptr;
  io.hit_out = w->events.hit_id;
  return io;
}

static hipError_t tdm_launch_step(const macm_tdm* w, const TdmBuffers& TB, int cur, const TdmIO& io, hipStream_t s) {
  if (w->wave) return launch_tdm_step_w64(w->P, w->B, w->TP, TB, cur, io, s);
  return launch_tdm_step_wg(w->P, w->B, w->TP, TB, cur, io, s);
}

static int tdm_init(macm_tdm* w, const macm_tdm_outputs* out, hipStream_t s) {
  HIP_TRY(hipStreamSynchronize(s));  // earlier steps' status stores land before the word is cleared
  clear_host_status(w->hstat);
  w->cur = 0;
  const TdmBuffers TB = tdm_with_outputs(w, out);
  HIP_TRY(tdm_launch_init(w, TB, out ? out->obs : nullptr, nullptr, s));
  if (out && out->done) HIP_TRY(hipMemsetAsync(out->done, 0, (size_t)w->P.n_envs, s));
  return MACM_OK;
}

int macm_tdm_reset(macm_tdm* w, uint64_t seed, int64_t env_offset, const macm_tdm_outputs* out, void* stream) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  DeviceGuard g(w->device);
  const macm_tdm_config& c = w->cfg;
  const int E = w->P.n_envs, N = w->P.n_agents;
  std::vector<float2> pos((size_t)E * N);
  std::vector<float> ang((size_t)E * N);
  std::vector<uint32_t> mts((size_t)E * kMtStride);
  for (int e = 0; e < E; ++e) {
    PyMT19937 r(seed + (uint64_t)(env_offset + e));
    for (int i = 0; i < N; ++i) {  // combat.py:80-95
      const double x = r.random() * (w->team[i] + c.world_width / 2);
      const double y = r.random() * c.world_height;
      const double a = r.uniform(-1, 1) * M_PI;
      pos[(size_t)e * N + i] = make_float2((float)x, (float)y);
      ang[(size_t)e * N + i] = (float)a;
    }
    save_stream(mts, e, r);
  }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(w->B.pos, pos.data(), pos.size() * sizeof(float2), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(w->B.angle, ang.data(), ang.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(w->mt, mts.data(), mts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  w->mt_valid = true;
  int rc = tdm_init(w, out, s);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));  // host vectors feed the async copies
  return MACM_OK;
}

int macm_tdm_place(macm_tdm* w, const void* pos, const void* angle, const macm_tdm_outputs* out, void* stream) {
  if (!w || !pos || !angle) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  const size_t EN = (size_t)w->P.n_envs * w->P.n_agents;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(w->B.pos, pos, EN * sizeof(float2), hipMemcpyDefault, s));
  HIP_TRY(hipMemcpyAsync(w->B.angle, angle, EN * sizeof(float), hipMemcpyDefault, s));
  w->mt_valid = false;  // poses came from the caller's generator
  int rc = tdm_init(w, out, s);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return MACM_OK;
}

static const char* const kNoTdmStreams = "no per-env random streams: the world was placed, not reset (macm_tdm_reset)";

static PoseDraw tdm_pose_draw(const macm_tdm* w) {
  PoseDraw D;
  memset(&D, 0, sizeof(D));
  D.mode = kTdm;
  D.n_agents = w->P.n_agents;
  D.half_width = w->cfg.world_width / 2;
  D.height = w->cfg.world_height;
  D.TP = w->TP;
  return D;
}

int macm_tdm_reset_envs(macm_tdm* w, const uint8_t* env_mask, const macm_tdm_outputs* out, void* stream) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  if (!w->mt_valid) return fail(MACM_E_INVALID, kNoTdmStreams);
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = fill_reset_mask(w->rmask, env_mask, w->P.n_envs, s);
  if (rc) return rc;
  HIP_TRY(launch_draw_poses(w->rmask, w->mt, tdm_pose_draw(w), w->P.n_envs, w->B.pos, w->B.angle, s));
  const TdmBuffers TB = tdm_with_outputs(w, out);
  HIP_TRY(tdm_launch_init(w, TB, out ? out->obs : nullptr, w->rmask, s));
  return resync_host_status(w->hstat, w->B.status, w->P.n_envs, s);
}

int macm_tdm_set_autoreset(macm_tdm* w, int32_t on) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  w->autoreset = on != 0;
  return MACM_OK;
}

int macm_tdm_set_final_outputs(macm_tdm* w, const macm_final_outputs* fin) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  FinalOut F;
  const int rc = final_outputs_from(fin, true, &F);
  if (rc) return rc;
  w->fin = F;
  return MACM_OK;
}

int macm_tdm_set_events(macm_tdm* w, const macm_tdm_events* ev) {
  const bool clear = !ev || !ev->hit_id;
  // the registration itself first: what it says is wrong whatever world it is for
  if (!clear && reinterpret_cast<uintptr_t>(ev->hit_id) % alignof(int32_t))
    return fail(MACM_E_INVALID, "events: hit_id must be 4-byte aligned");
  if (!clear && ev->rows < 1) return fail(MACM_E_INVALID, "events: rows must be >= 1");
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  w->events = clear ? macm_tdm_events{nullptr, 0} : *ev;
  return MACM_OK;
}

// A macm_tdm_policy as the kernels can take it
static int tdm_policy_check(const macm_tdm_policy* p) {
  if (p->hidden != 16 && p->hidden != 32) return fail(MACM_E_INVALID, "tdm policy: hidden must be 16 or 32");
  for (int i = 0; i < 3; ++i)
    if (p->reserved[i] != 0) return fail(MACM_E_INVALID, "tdm policy: reserved must be 0");
  if (!p->params) return fail(MACM_E_INVALID, "tdm policy: params is NULL");
  if (reinterpret_cast<uintptr_t>(p->params) & 15) return fail(MACM_E_INVALID, "tdm policy: params must be 16-byte aligned");
  return MACM_OK;
}

int macm_policy_tdm(const macm_tdm_policy* p, const void* obs, const uint8_t* mask, const double* health,
                    int32_t obs_f64, int32_t n_agents, int64_t rows, const uint8_t* agents, const float* noise,
                    uint8_t* actions, float* logits, void* stream) {
  if (!p) return fail(MACM_E_INVALID, "tdm policy is NULL");
  if (const int rc = tdm_policy_check(p)) return rc;
  if (!obs || !mask || !health || !actions) return fail(MACM_E_INVALID, "obs/mask/health/actions is NULL");
  if (reinterpret_cast<uintptr_t>(obs) & 15) return fail(MACM_E_INVALID, "obs must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(actions) & 3) return fail(MACM_E_INVALID, "actions must be 4-byte aligned");
  if (n_agents < 2) return fail(MACM_E_INVALID, "n_agents must be >= 2");
  if (rows < 0) return fail(MACM_E_INVALID, "rows must be >= 0");
  if (rows % n_agents != 0)
    return fail(MACM_E_INVALID, "rows must be a multiple of n_agents (rows = E * N: row r is agent r % n_agents)");
  const TdmPolicyArgs M{p->params, noise, logits, p->hidden, 0u};
  HIP_TRY(launch_policy_tdm(M, obs, mask, health, obs_f64 != 0, n_agents, rows, agents, nullptr, 0.0, actions,
                            (hipStream_t)stream));
  return MACM_OK;
}

// The workspace of macm_tdm_policy_grad: one partial of the larger net per wave
static int64_t tdm_grad_workspace_bytes(int64_t rows) {
  return (int64_t)mlp_grad_partials(rows) * tdm_policy_n_params(32) * (int64_t)sizeof(float);
}

int macm_tdm_grad_workspace(int64_t rows, int64_t* bytes) {
  if (!bytes) return fail(MACM_E_INVALID, "tdm grad: bytes is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "tdm grad: rows must be >= 0");
  *bytes = tdm_grad_workspace_bytes(rows);
  return MACM_OK;
}

int macm_tdm_policy_grad(const macm_tdm_policy* p, const void* obs, const uint8_t* mask, const double* health,
                         int32_t obs_f64, int32_t n_agents, int64_t rows, const uint8_t* agents, const float* dlogits,
                         float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p) return fail(MACM_E_INVALID, "tdm policy is NULL");
  if (const int rc = tdm_policy_check(p)) return rc;
  if (!obs || !mask || !health) return fail(MACM_E_INVALID, "tdm grad: obs/mask/health is NULL");
  if (!dlogits || !grad) return fail(MACM_E_INVALID, "tdm grad: dlogits/grad is NULL");
  if (reinterpret_cast<uintptr_t>(obs) & 15) return fail(MACM_E_INVALID, "tdm grad: obs must be 16-byte aligned");
  if (n_agents < 2) return fail(MACM_E_INVALID, "tdm grad: n_agents must be >= 2");
  if (rows < 0) return fail(MACM_E_INVALID, "tdm grad: rows must be >= 0");
  if (rows % n_agents != 0)
    return fail(MACM_E_INVALID,
                "tdm grad: rows must be a multiple of n_agents (rows = E * N: row r is agent r % n_agents)");
  if (rows > 0 && !workspace) return fail(MACM_E_INVALID, "tdm grad: workspace is NULL");
  if (rows > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail(MACM_E_INVALID, "tdm grad: workspace must be 16-byte aligned");
  if (rows > 0 && workspace_bytes < tdm_grad_workspace_bytes(rows))
    return fail(MACM_E_INVALID, "tdm grad: workspace_bytes " + std::to_string(workspace_bytes) + " is below the " +
                                    std::to_string(tdm_grad_workspace_bytes(rows)) + " of macm_tdm_grad_workspace");
  const TdmPolicyArgs M{p->params, nullptr, nullptr, p->hidden, 0u};
  HIP_TRY(launch_tdm_policy_grad(M, obs, mask, health, obs_f64 != 0, n_agents, rows, agents, dlogits, grad,
                                 (float*)workspace, (hipStream_t)stream));
  return MACM_OK;
}

int macm_tdm_set_policy(macm_tdm* w, const macm_tdm_policy* p, uint32_t team_mask) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  if (!p) {
    w->policy = macm_tdm_policy{0, {0, 0, 0}, nullptr};
    w->policy_teams = 0;
    w->policy_all = false;
    return MACM_OK;
  }
  if (const int rc = tdm_policy_check(p)) return rc;
  if (team_mask == 0) return fail(MACM_E_INVALID, "tdm policy: team_mask is 0 (no team would take the policy)");
  if (team_mask >> w->cfg.n_teams)
    return fail(MACM_E_INVALID, "tdm policy: team_mask names a team at or above n_teams = " + std::to_string(w->cfg.n_teams));
  DeviceGuard g(w->device);
  const int N = w->P.n_agents;
  std::vector<uint8_t> ag(N);
  bool all = true;
  for (int i = 0; i < N; ++i) {
    ag[i] = (team_mask >> w->team[i]) & 1u;
    all = all && ag[i];
  }
  if (!w->policy_agents)
    if (const int rc = dalloc(w->allocs, &w->policy_agents, (size_t)N)) return rc;
  HIP_TRY(hipDeviceSynchronize());  // a launch in flight may still read the mask of the registration before
  HIP_TRY(hipMemcpy(w->policy_agents, ag.data(), (size_t)N, hipMemcpyHostToDevice));
  w->policy = *p;
  w->policy_teams = team_mask;
  w->policy_all = all;
  return MACM_OK;
}

// As world_autoreset_step: the step's done flags (a private copy) mask the draw and init launches.
// TB / obs: the step's outputs; the init writes the new initial obs and mask there and leaves the
// terminal health, alive and winner outputs as the step wrote them.
static int tdm_autoreset_step(macm_tdm* w, const TdmBuffers& TB, void* obs, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(w->rmask, w->B.done, (size_t)w->P.n_envs, hipMemcpyDeviceToDevice, s));
  if (w->fin.any()) {  // the rows the init overwrites, into the registered final outputs first
    const size_t S = (size_t)w->P.n_agents * (w->P.n_agents - 1);
    FinalRows rows;
    rows.obs = obs;
    rows.obs_bytes = S * 4 * (w->cfg.obs_f64 ? sizeof(double) : sizeof(float));
    rows.msk = TB.mask_out;
    rows.n_msk = (int)S;
    HIP_TRY(launch_final_copy(w->rmask, w->fin, rows, w->B.step_count, w->P.n_envs, s));
  }
  HIP_TRY(launch_draw_poses(w->rmask, w->mt, tdm_pose_draw(w), w->P.n_envs, w->B.pos, w->B.angle, s));
  TdmBuffers TBi = TB;
  TBi.health_out = nullptr;
  TBi.alive_out = nullptr;
  TBi.winner_out = nullptr;
  TBi.snap_out = nullptr;
  HIP_TRY(tdm_launch_init(w, TBi, obs, w->rmask, s));
  return MACM_OK;
}

// The split observation (round 6, tdm_obs_snap.hip). The wave kernel (N <= 64) observes on its one
// wave after the physics: 55% of its cycles at 2 x 16 (tools/tdm_phase.py). With fewer envs than
// SIMDs (BASELINE C4's per-GPU shard: 512 envs, 0.5 waves per SIMD) that observation is one wave's
// latency chain. Split, the step writes pose snapshots and tdm_observe_snap observes every
// (step, env) row with a workgroup of its own; a trajectory rollout runs in chunks of
// kTdmSplitChunk steps, each chunk's observation on a second stream beside the next chunk's physics.
// Bit-identical either way. Measured (profiles/r06/split/, 2 x 16, one box): 512 envs 13.2 -> 11.6 us
// per step at steady state, 18.8 -> 18.1 us in the driver's window; 1024 envs even; 2048 and 4096 envs
// slower (26 / 50 us against 20 / 28: with every SIMD busy the observation kernel only competes with
// the physics). The physics alone takes ~11 us per step at 512 envs (rocprof: the chunk launches),
// one wave's latency chain, which bounds the shard whatever the observation costs.
// Below kTdmSplitMaxEnvs envs by default; MACM_TDM_SPLIT_OBS=0/1 overrides
// (tests, A/B). The closed loop (the bots read each step's observation inside the launch) and the
// workgroup step (N > 64) keep the fused form.
static constexpr int kTdmSplitMaxEnvs = 1024, kTdmSplitChunk = 8;

static bool tdm_split_obs(const macm_tdm* w) {
  if (!w->wave || w->autoreset) return false;  // autoreset: the observation inside the step
  const char* v = getenv("MACM_TDM_SPLIT_OBS");
  return v ? atoi(v) != 0 : w->P.n_envs < kTdmSplitMaxEnvs;
}

// snapshot halves of at least `rows` rows each (grown on demand; the caller's stream has finished
// every earlier use: each split call ends with the stream joined to the observation stream)
static int tdm_split_buffers(macm_tdm* w, size_t rows, hipStream_t s) {
  if (!w->obs_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&w->obs_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIP_TRY(hipEventCreateWithFlags(&w->ev_phys[b], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&w->ev_obs[b], hipEventDisableTiming));
    }
  }
  if (rows > w->snap_rows) {
    // at least a whole chunk's rows at the first allocation (a warm-up rollout shorter than a chunk
    // would otherwise leave the next rollout a synchronising reallocation)
    const size_t chunk = (size_t)kTdmSplitChunk * w->P.n_envs;
    if (rows < chunk) rows = chunk;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamSynchronize(w->obs_stream));
    if (w->snap) HIP_TRY(hipFree(w->snap));
    w->snap = nullptr;
    w->snap_rows = 0;
    if (hipMalloc(&w->snap, 2 * rows * (size_t)w->P.n_agents * sizeof(float4)) != hipSuccess) {
      (void)hipGetLastError();
      w->snap = nullptr;
      return fail(MACM_E_OOM, "hipMalloc (split observation snapshots)");
    }
    w->snap_rows = rows;
  }
  return MACM_OK;
}

int macm_tdm_step(macm_tdm* w, const void* actions, const macm_tdm_outputs* out, void* stream) {
  if (!w || !actions) return fail(MACM_E_INVALID, "tdm/actions is NULL");
  if (w->autoreset && !w->mt_valid) return fail(MACM_E_INVALID, kNoTdmStreams);
  if (const int rc = final_outputs_need(w->autoreset, w->fin, out ? out->obs : nullptr, nullptr,
                                        out ? out->mask : nullptr))
    return rc;
  if (const uint32_t st = read_host_status(w->hstat)) return overflow_error(st);
  DeviceGuard g(w->device);
  if (w->cfg.validate_actions) {
    const int rc = check_actions(w->bad, actions, 2, w->TB.alive, w->P.n_envs, w->P.n_agents, (hipStream_t)stream);
    if (rc) return rc;
  }
  TdmBuffers TB = tdm_with_outputs(w, out);
  hipStream_t s = (hipStream_t)stream;
  TdmIO io = tdm_io(w, actions, out);
  void* const obs = io.obs;
  if ((obs || TB.mask_out) && tdm_split_obs(w)) {
    const int rc = tdm_split_buffers(w, (size_t)w->P.n_envs, s);
    if (rc) return rc;
    TB.snap_out = w->snap;
    io.obs = nullptr;  // the step writes pose snapshots, tdm_observe_snap the observation
    HIP_TRY(tdm_launch_step(w, TB, w->cur, io, s));
    w->cur ^= 1;
    HIP_TRY(launch_tdm_observe_snap(w->TP, w->P.n_agents, (size_t)w->P.n_envs, w->snap, obs, w->cfg.obs_f64 != 0,
                                    TB.mask_out, s));
    return MACM_OK;
  }
  HIP_TRY(tdm_launch_step(w, TB, w->cur, io, s));
  w->cur ^= 1;
  if (w->autoreset) return tdm_autoreset_step(w, TB, obs, s);
  return MACM_OK;
}

// The tail observation (flock_step_w64.hip TailObs): a trajectory rollout of the wave kernel whose
// launch is wholly resident (the envs plus the observe-only blocks within the kernel's occupancy on
// this device). MACM_TDM_TAIL_OBS=0/1 overrides the default; MACM_TDM_TAIL_WORKERS sets the number
// of observe-only blocks (default: as many as the envs, within the resident capacity).
static int tdm_tail_workers(macm_tdm* w) {
  if (!w->wave) return -1;
  if (w->tail_cap < 0) w->tail_cap = tdm_rollout_resident_blocks(w->P.n_agents, w->cfg.obs_f64 != 0);
  const int E = w->P.n_envs, room = w->tail_cap - E;
  if (room < 0) return -1;
  const char* v = getenv("MACM_TDM_TAIL_WORKERS");
  int x = v ? atoi(v) : E;
  if (x < 0) x = 0;
  return x < room ? x : room;
}

// measured (profiles/r06/tail/): 512-1536 envs faster than the fused and split forms (C4 shard steady
// 13.3 -> 7.35 us, window 17.9 -> 15.3 us; 1536 envs window -3.4%), 2048 envs +4% and 4096 +24% in
// the window (the chip is full of physics waves, so the observation waits for the tail)
static constexpr int kTdmTailMaxEnvs = 2048;
static constexpr int kTdmSnapMinSteps = 32;  // the tail observation's first snapshot allocation, in steps
static bool tdm_tail_obs(macm_tdm* w) {
  if (w->autoreset) return false;  // the tail's pose snapshots know nothing of a mid-launch respawn
  const char* v = getenv("MACM_TDM_TAIL_OBS");
  if (v ? atoi(v) == 0 : w->P.n_envs >= kTdmTailMaxEnvs) return false;
  return tdm_tail_workers(w) >= 0;
}

// The steps observed in the tail: all below kTdmTailMaxEnvs; from there only the last
// MACM_TDM_TAIL_STEPS (the earlier steps observe in the step, the fused form), so that the observation
// of the last steps runs in the launch's tail while the heaviest envs finish
static int tdm_tail_k0(const macm_tdm* w, int n_steps) {
  int steps = w->P.n_envs >= kTdmTailMaxEnvs ? n_steps / 4 : n_steps;
  if (const char* v = getenv("MACM_TDM_TAIL_STEPS")) steps = atoi(v);
  if (steps < 1) steps = 1;
  if (steps > n_steps) steps = n_steps;
  return n_steps - steps;
}

// the tail observation's snapshot rows, grown rarely: a first allocation covers rollouts of up to
// kTdmSnapMinSteps steps, so that a short warm-up rollout does not leave the next, longer one a
// synchronising reallocation (macm_tdm_reserve sizes it ahead for longer ones)
static int tdm_tail_snapshots(macm_tdm* w, size_t rows, hipStream_t s) {
  if (rows <= w->tail_rows) return MACM_OK;
  const size_t E = w->P.n_envs, N = w->P.n_agents;
  const size_t want = rows > (size_t)kTdmSnapMinSteps * E ? rows : (size_t)kTdmSnapMinSteps * E;
  HIP_TRY(hipStreamSynchronize(s));
  if (w->tail_snap) HIP_TRY(hipFree(w->tail_snap));
  w->tail_snap = nullptr;
  w->tail_rows = 0;
  if (hipMalloc(&w->tail_snap, want * N * sizeof(float4)) != hipSuccess) {
    (void)hipGetLastError();
    w->tail_snap = nullptr;
    return fail(MACM_E_OOM, "hipMalloc (tail observation snapshots)");
  }
  w->tail_rows = want;
  return MACM_OK;
}

static int tdm_rollout_tail(macm_tdm* w, const TdmBuffers& TB, const TdmIO& io, const RollShape& sh, hipStream_t s) {
  const int n_steps = sh.nsteps, k0 = tdm_tail_k0(w, n_steps);
  const size_t E = w->P.n_envs, rows = (size_t)(n_steps - k0) * E;
  if (!w->tail_ctl) {
    if (hipMalloc(&w->tail_ctl, tail_ctl_words((int)E) * sizeof(unsigned long long)) != hipSuccess) {
      (void)hipGetLastError();
      w->tail_ctl = nullptr;
      return fail(MACM_E_OOM, "hipMalloc (tail observation counters)");
    }
    HIP_TRY(hipMemsetAsync(w->tail_ctl, 0, tail_ctl_words((int)E) * sizeof(unsigned long long), s));
    w->tail_tag = 0;
  }
  if (const int rc = tdm_tail_snapshots(w, rows, s)) return rc;
  if (++w->tail_tag == 0) w->tail_tag = 1;  // tags are > 0: a ready word of 0 never matches
  TdmBuffers TBt = TB;
  TBt.snap_out = w->tail_snap;
  TailLaunch tail;
  tail.ctl = w->tail_ctl;
  tail.tag = w->tail_tag;
  tail.workers = tdm_tail_workers(w);
  tail.k0 = k0;
  HIP_TRY(launch_tdm_rollout_w64(w->P, w->B, w->TP, TBt, w->cur, io, sh, tail, s));
  if (n_steps & 1) w->cur ^= 1;
  return MACM_OK;
}

// A wave-kernel rollout (not the closed loop) with the split observation: the overwrite form keeps
// one snapshot row per env (the last step's) and observes it once; the trajectory form steps
// chunks of kTdmSplitChunk steps into alternating snapshot halves, each chunk observed on the
// observation stream while the caller's stream steps the next chunk.
static int tdm_rollout_split(macm_tdm* w, const TdmBuffers& TB, const TdmIO& io, const RollShape& sh, hipStream_t s) {
  const size_t E = w->P.n_envs, N = w->P.n_agents, EN = E * N, S = N - 1;
  const bool f64 = io.obs_f64;
  const int n_steps = sh.nsteps;
  TdmIO phys = io;  // the physics launches: no observation (the pose snapshots instead)
  phys.obs = nullptr;
  const size_t orow = EN * S * 4 * (f64 ? sizeof(double) : sizeof(float));  // obs bytes per step
  if (!sh.traj) {
    int rc = tdm_split_buffers(w, E, s);
    if (rc) return rc;
    TdmBuffers TBs = TB;
    TBs.snap_out = w->snap;
    HIP_TRY(launch_tdm_rollout_w64(w->P, w->B, w->TP, TBs, w->cur, phys, sh, TailLaunch{}, s));
    if (n_steps & 1) w->cur ^= 1;
    HIP_TRY(launch_tdm_observe_snap(w->TP, (int)N, E, w->snap, io.obs, f64, TB.mask_out, s));
    return MACM_OK;
  }
  const int KC = n_steps < kTdmSplitChunk ? n_steps : kTdmSplitChunk;
  int rc = tdm_split_buffers(w, (size_t)KC * E, s);
  if (rc) return rc;
  const unsigned char* act = static_cast<const unsigned char*>(io.actions);
  unsigned char* obs = static_cast<unsigned char*>(io.obs);
  RollShape chunk = sh;
  int c = 0;
  for (int k0 = 0; k0 < n_steps; k0 += KC, ++c) {
    const int kc = n_steps - k0 < KC ? n_steps - k0 : KC, b = c & 1;
    float4* snap = w->snap + (size_t)b * w->snap_rows * N;
    if (c >= 2) HIP_TRY(hipStreamWaitEvent(s, w->ev_obs[b], 0));  // chunk c - 2's observation has read this half
    TdmBuffers TBc = TB;
    auto row = [k0](auto* p, size_t per) { return p ? p + (size_t)k0 * per : p; };
    TBc.mask_out = nullptr;
    TBc.health_out = row(TB.health_out, EN);
    TBc.alive_out = row(TB.alive_out, EN);
    TBc.winner_out = row(TB.winner_out, E);
    TBc.snap_out = snap;
    phys.actions = act + (size_t)k0 * sh.astride;
    phys.done = row(io.done, E);
    phys.hit_out = row(io.hit_out, EN);
    chunk.nsteps = kc;
    HIP_TRY(launch_tdm_rollout_w64(w->P, w->B, w->TP, TBc, w->cur, phys, chunk, TailLaunch{}, s));
    if (kc & 1) w->cur ^= 1;
    HIP_TRY(hipEventRecord(w->ev_phys[b], s));
    HIP_TRY(hipStreamWaitEvent(w->obs_stream, w->ev_phys[b], 0));
    HIP_TRY(launch_tdm_observe_snap(w->TP, (int)N, (size_t)kc * E, snap, obs ? obs + (size_t)k0 * orow : nullptr, f64,
                                    row(TB.mask_out, EN * S), w->obs_stream));
    HIP_TRY(hipEventRecord(w->ev_obs[b], w->obs_stream));
  }
  // joined: the caller's stream waits for the last chunk's observation (the stream is in order)
  HIP_TRY(hipStreamWaitEvent(s, w->ev_obs[(c - 1) & 1], 0));
  return MACM_OK;
}

// macm_tdm_rollout / _traj (bots = false), macm_tdm_rollout_bots / _traj (bots = true) and
// macm_tdm_rollout_policy / _traj (bots = true, pol: the registered policy's params and teams and this
// call's noise and logits; the other teams' agents keep the bot)
static int tdm_rollout(macm_tdm* w, const void* actions, int n_steps, const macm_tdm_outputs* out, void* stream,
                       bool bots, bool traj, const TdmPolicyArgs* pol = nullptr) {
  if (n_steps < 0) return fail(MACM_E_INVALID, "n_steps must be >= 0");
  if (n_steps == 0) return MACM_OK;
  if (!w || !actions) return fail(MACM_E_INVALID, "tdm/actions is NULL");
  if ((bots || traj) && !out) return fail(MACM_E_INVALID, "out is NULL");
  if (bots && (!out->obs || !out->mask)) return fail(MACM_E_INVALID, "out->obs/mask is NULL (the bots act on them)");
  if (pol && !out->health) return fail(MACM_E_INVALID, "out->health is NULL (the policy reads it)");
  if (w->autoreset && !w->mt_valid) return fail(MACM_E_INVALID, kNoTdmStreams);
  if (const int rc = final_outputs_need(w->autoreset, w->fin, out ? out->obs : nullptr, nullptr,
                                        out ? out->mask : nullptr))
    return rc;
  if (traj && w->events.hit_id && n_steps > w->events.rows)
    return fail(MACM_E_INVALID, "events: n_steps " + std::to_string(n_steps) + " exceeds the " +
                                    std::to_string(w->events.rows) + " rows registered (macm_tdm_set_events)");
  if (const uint32_t st = read_host_status(w->hstat)) return overflow_error(st);
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  if (w->cfg.validate_actions) {
    // bots: the caller's first step, alive agents; else every agent's actions of every step, alive
    // or not (deaths are not known yet)
    const long long rows = (long long)(bots ? 1 : n_steps) * w->P.n_envs;
    if (rows > INT32_MAX) return fail(MACM_E_INVALID, "n_steps * n_envs too large to validate");
    const int rc =
        check_actions(w->bad, actions, 2, bots ? w->TB.alive : nullptr, (int)rows, w->P.n_agents, s, w->P.n_envs);
    if (rc) return rc;
  }
  const TdmBuffers TB = tdm_with_outputs(w, out);
  const unsigned long long astride = bots ? 0ull : (unsigned long long)w->P.n_envs * w->P.n_agents * 4;
  TdmIO io = tdm_io(w, actions, out);
  io.policy = pol;
  const RollShape sh(n_steps, astride, traj);
  if (!w->wave) {
    // workgroup step (N > 64): one launch per step (and the bots kernel's), in order; trajectory
    // form: step k's outputs in row k of [K, ...], the closed loop reading action row k and the bot
    // writing row k + 1 of [K + 1, E, N, 4]
    const size_t E = w->P.n_envs, N = w->P.n_agents, EN = E * N;
    const size_t obytes = EN * (N - 1) * 4 * (w->cfg.obs_f64 ? sizeof(double) : sizeof(float));
    const unsigned long long kstride = bots ? (traj ? EN * 4 : 0ull) : astride;
    const unsigned char* act = static_cast<const unsigned char*>(actions);
    for (int k = 0; k < n_steps; ++k) {
      const size_t kr = traj ? (size_t)k : 0;
      TdmBuffers TBk = TB;
      auto row = [kr](auto* p, size_t per) { return p ? p + kr * per : p; };
      TBk.mask_out = row(TB.mask_out, EN * (N - 1));
      TBk.health_out = row(TB.health_out, EN);
      TBk.alive_out = row(TB.alive_out, EN);
      TBk.winner_out = row(TB.winner_out, E);
      void* obs_k = io.obs ? static_cast<unsigned char*>(io.obs) + kr * obytes : nullptr;
      const unsigned char* act_k = act + k * kstride;
      TdmIO iok = io;
      iok.actions = act_k;
      iok.obs = obs_k;
      iok.done = row(io.done, E);
      iok.hit_out = row(io.hit_out, EN);
      HIP_TRY(tdm_launch_step(w, TBk, w->cur, iok, s));
      w->cur ^= 1;
      if (w->autoreset) {  // before the bots: a reset env's next actions come from its new initial obs
        const int rc = tdm_autoreset_step(w, TBk, obs_k, s);
        if (rc) return rc;
      }
      unsigned char* const next = const_cast<unsigned char*>(act_k) + (traj ? EN * 4 : 0);
      if (bots && !(pol && w->policy_all))
        HIP_TRY(launch_bots_combat(obs_k, TBk.mask_out, w->cfg.obs_f64 != 0, (int)N, (long long)EN, next, s));
      if (pol) {  // over the bot's actions: the rows of the policy's teams, noise row k, the logits into the step's row
        TdmPolicyArgs M = *pol;
        if (M.noise) M.noise += (size_t)k * EN * kTdmPolicyLogits;
        if (M.logits) M.logits += kr * EN * kTdmPolicyLogits;
        // (autoreset: rmask holds this step's done flags; a reset env's health output keeps the terminal health)
        HIP_TRY(launch_policy_tdm(M, obs_k, TBk.mask_out, TBk.health_out, w->cfg.obs_f64 != 0, (int)N, (long long)EN,
                                  w->policy_all ? nullptr : w->policy_agents, w->autoreset ? w->rmask : nullptr,
                                  w->TP.init_health, next, s));
      }
    }
    return MACM_OK;
  }
  if (!bots && traj && out && (out->obs || out->mask) && tdm_tail_obs(w))
    return tdm_rollout_tail(w, TB, io, sh, s);
  if (!bots && out && (out->obs || out->mask) && tdm_split_obs(w))
    return tdm_rollout_split(w, TB, io, sh, s);
  if (w->autoreset)  // the kernels with the in-launch reset (the observation inside the step)
    HIP_TRY(launch_tdm_rollout_ar_w64(w->P, w->B, w->TP, TB, w->cur, io, sh,
                                      ResetLaunch(w->mt, tdm_pose_draw(w), w->fin), s));
  else
    HIP_TRY(launch_tdm_rollout_w64(w->P, w->B, w->TP, TB, w->cur, io, sh, TailLaunch{}, s));
  if (n_steps & 1) w->cur ^= 1;
  return MACM_OK;
}

int macm_tdm_rollout(macm_tdm* w, const void* actions, int n_steps, const macm_tdm_outputs* out, void* stream) {
  return tdm_rollout(w, actions, n_steps, out, stream, false, false);
}

int macm_tdm_rollout_traj(macm_tdm* w, const void* actions, int n_steps, const macm_tdm_outputs* traj,
                          void* stream) {
  return tdm_rollout(w, actions, n_steps, traj, stream, false, true);
}

int macm_tdm_rollout_bots(macm_tdm* w, uint8_t* actions, int n_steps, const macm_tdm_outputs* out, void* stream) {
  return tdm_rollout(w, actions, n_steps, out, stream, true, false);
}

int macm_tdm_rollout_bots_traj(macm_tdm* w, uint8_t* actions, int n_steps, const macm_tdm_outputs* traj,
                               void* stream) {
  return tdm_rollout(w, actions, n_steps, traj, stream, true, true);
}

static int tdm_rollout_policy(macm_tdm* w, uint8_t* actions, int n_steps, const float* noise, float* logits,
                              const macm_tdm_outputs* out, void* stream, bool traj) {
  if (n_steps < 0) return fail(MACM_E_INVALID, "n_steps must be >= 0");
  if (n_steps == 0) return MACM_OK;
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  if (!w->policy.params) return fail(MACM_E_INVALID, "no policy is registered (macm_tdm_set_policy)");
  const TdmPolicyArgs M{w->policy.params, noise, logits, w->policy.hidden, w->policy_teams};
  return tdm_rollout(w, actions, n_steps, out, stream, true, traj, &M);
}

int macm_tdm_rollout_policy(macm_tdm* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                            const macm_tdm_outputs* out, void* stream) {
  return tdm_rollout_policy(w, actions, n_steps, noise, logits, out, stream, false);
}

int macm_tdm_rollout_policy_traj(macm_tdm* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                                 const macm_tdm_outputs* traj, void* stream) {
  return tdm_rollout_policy(w, actions, n_steps, noise, logits, traj, stream, true);
}

int macm_tdm_observe(macm_tdm* w, const macm_tdm_outputs* out, void* stream) {
  if (!w || !out) return fail(MACM_E_INVALID, "tdm/out is NULL");
  DeviceGuard g(w->device);
  const TdmBuffers TB = tdm_with_outputs(w, out);
  if (w->wave)
    HIP_TRY(launch_tdm_observe_w64(w->P, w->B, w->TP, TB, out->obs, w->cfg.obs_f64 != 0, (hipStream_t)stream));
  else
    HIP_TRY(launch_tdm_observe_wg(w->P, w->B, w->TP, TB, out->obs, w->cfg.obs_f64 != 0, (hipStream_t)stream));
  hipStream_t s = (hipStream_t)stream;
  const size_t EN = (size_t)w->P.n_envs * w->P.n_agents, E = (size_t)w->P.n_envs;
  if (out->health) HIP_TRY(hipMemcpyAsync(out->health, w->TB.health, EN * sizeof(double), hipMemcpyDefault, s));
  if (out->alive) HIP_TRY(hipMemcpyAsync(out->alive, w->TB.alive, EN, hipMemcpyDefault, s));
  if (out->done) HIP_TRY(hipMemcpyAsync(out->done, w->B.done, E, hipMemcpyDefault, s));
  if (out->winner) HIP_TRY(hipMemcpyAsync(out->winner, w->TB.winner, E * sizeof(int32_t), hipMemcpyDefault, s));
  return MACM_OK;
}

static int tdm_copy_state(macm_tdm* w, const macm_tdm_state* st, void* stream, bool to_device) {
  if (!w || !st) return fail(MACM_E_INVALID, "tdm/state is NULL");
  if (st->contact_stride < 0) return fail(MACM_E_INVALID, "contact_stride must be >= 0");
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t E = w->P.n_envs, N = w->P.n_agents;
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
      {st->health, w->TB.health, E * N * sizeof(double)},
      {st->cd_atk, w->TB.cd_atk, E * N * sizeof(double)},
      {st->cd_mov, w->TB.cd_mov, E * N * sizeof(double)},
      {st->alive, w->TB.alive, E * N},
      {st->listener, w->TB.listener, E * sizeof(int2)},
      {st->step_count, w->B.step_count, E * sizeof(int32_t)},
      {st->time_passed, w->B.time_passed, E * sizeof(double)},
      {st->done, w->B.done, E},
      {st->winner, w->TB.winner, E * sizeof(int32_t)},
  };
  if (const int rc = copy_state_lists(w, st, to_device, s)) return rc;
  for (const Item& it : items) {
    if (!it.user) continue;
    if (to_device) HIP_TRY(hipMemcpyAsync(it.dev, it.user, it.bytes, hipMemcpyDefault, s));
    else HIP_TRY(hipMemcpyAsync(it.user, it.dev, it.bytes, hipMemcpyDefault, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return MACM_OK;
}

int macm_tdm_get_state(macm_tdm* w, const macm_tdm_state* dst, void* stream) {
  return tdm_copy_state(w, dst, stream, false);
}

int macm_tdm_set_state(macm_tdm* w, const macm_tdm_state* src, void* stream) {
  return tdm_copy_state(w, src, stream, true);
}

int macm_tdm_status(macm_tdm* w, int32_t* status_or, void* stream) { return world_status(w, status_or, stream); }

int macm_tdm_counters(macm_tdm* w, int64_t out[4], void* stream) { return world_counters(w, out, stream); }

int macm_tdm_launch_flags(const macm_tdm* w) {
  if (!w) return fail(MACM_E_INVALID, "tdm is NULL");
  return (tdm_split_obs(w) ? MACM_LAUNCH_SPLIT_OBS : 0) |
         (tdm_tail_obs(const_cast<macm_tdm*>(w)) ? MACM_LAUNCH_TAIL_OBS : 0);
}

int macm_tdm_reserve(macm_tdm* w, int32_t n_steps, void* stream) {
  if (!w || n_steps < 0) return fail(MACM_E_INVALID, "tdm is NULL or n_steps < 0");
  DeviceGuard g(w->device);
  if (!tdm_tail_obs(w) || n_steps == 0) return MACM_OK;
  const int k0 = tdm_tail_k0(w, n_steps);
  return tdm_tail_snapshots(w, (size_t)(n_steps - k0) * w->P.n_envs, (hipStream_t)stream);
}

int macm_tdm_spilled(macm_tdm* w, int64_t* env_steps, void* stream) { return world_spilled(w, env_steps, stream); }

int macm_tdm_set_debug(macm_tdm* w, int32_t flags) {
  if (!w) return fail(MACM_E_INVALID, "world is NULL");
  const int pool = (flags & MACM_DEBUG_SPILL_POOL) ? (flags >> 8) : 0;
  flags &= 0xff;
  if (flags & ~(MACM_DEBUG_FORCE_SPILL | MACM_DEBUG_SPILL_POOL | MACM_DEBUG_SPILL_FAIL))
    return fail(MACM_E_INVALID, "unknown debug flag (TDM: FORCE_SPILL, SPILL_POOL, SPILL_FAIL)");
  if (int rc = set_spill_pool(w, flags, pool)) return rc;
  w->P.force_spill = (flags & MACM_DEBUG_FORCE_SPILL) ? 1 : 0;
  return MACM_OK;
}

#ifdef MACM_STAMPS
// Diagnostic build only: copy the per-env phase stamps [E, 32] of the last step (the wave kernel
// uses rows of 16).
int macm_debug_tdm_stamps(macm_tdm* w, unsigned long long* out) {
  if (!w || !out) return fail(MACM_E_INVALID, "NULL argument");
  DeviceGuard g(w->device);
  HIP_TRY(hipMemcpy(out, w->B.stamps, (size_t)w->P.n_envs * 32 * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost));
  return MACM_OK;
}
#endif

}  // extern "C"
