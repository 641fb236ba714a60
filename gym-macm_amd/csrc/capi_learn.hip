// capi_learn.hip — the stateless part of the C-ABI of libmacm_hip.so (declared in include/macm.h): the
// version and last-error calls, the one-shot policy, value and GAE kernels, the gradients, the PPO loss
// and the scripted actors. No world, no torch types, no exceptions across the ABI.
#include "capi_common.hpp"

static thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

extern "C" {

const char* macm_version(void) {
  return "macm-hip 0.6.0 (gfx950; Flock: wave-per-env kernel N<=64, workgroup-per-env kernels N<=1024, "
         "spill step for dense envs and N<=4096; TDM: wave-per-env kernel N<=64, workgroup step N<=4096)";
}
int macm_abi_version(void) { return MACM_ABI_VERSION; }
const char* macm_last_error(void) { return g_last_error.c_str(); }

int macm_policy_flock(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows, const float* noise,
                      uint8_t* actions, float* logits, void* stream) {
  if (!p) return fail(MACM_E_INVALID, "policy is NULL");
  if (const int rc = mlp_check("policy", p)) return rc;
  if (!obs || !actions) return fail(MACM_E_INVALID, "obs/actions is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "rows must be >= 0");
  const PolicyArgs M{p->params, noise, logits, p->hidden, p->n_hidden};
  HIP_TRY(launch_policy_flock(M, obs, obs_f64 != 0, p->in_dim, rows, actions, (hipStream_t)stream));
  return MACM_OK;
}

int macm_policy_noise_at(const macm_sample_config* cfg, int64_t first_row, int64_t n_dec, int64_t rows, float* noise,
                         uint32_t* words, void* stream) {
  if (const int rc = sample_check(cfg, rows, first_row)) return rc;
  if (n_dec < 0) return fail(MACM_E_INVALID, "sampling: n_dec must be >= 0");
  if (!noise) return fail(MACM_E_INVALID, "sampling: noise is NULL");
  HIP_TRY(launch_policy_noise(SampleArgs{cfg->seed, cfg->decision, (uint32_t)first_row}, n_dec, rows, noise, words,
                              (hipStream_t)stream));
  return MACM_OK;
}

int macm_policy_noise(const macm_sample_config* cfg, int64_t n_dec, int64_t rows, float* noise, uint32_t* words,
                      void* stream) {
  return macm_policy_noise_at(cfg, 0, n_dec, rows, noise, words, stream);
}

int macm_policy_flock_sampled_at(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t first_row,
                                 int64_t rows, const macm_sample_config* cfg, uint8_t* actions, float* logits,
                                 void* stream) {
  if (!p) return fail(MACM_E_INVALID, "policy is NULL");
  if (const int rc = mlp_check("policy", p)) return rc;
  if (!obs || !actions) return fail(MACM_E_INVALID, "obs/actions is NULL");
  if (const int rc = sample_check(cfg, rows, first_row)) return rc;
  const PolicyArgs M{p->params, nullptr, logits, p->hidden, p->n_hidden};
  HIP_TRY(launch_policy_flock_sampled(M, SampleArgs{cfg->seed, cfg->decision, (uint32_t)first_row}, obs, obs_f64 != 0,
                                      p->in_dim, rows, actions, (hipStream_t)stream));
  return MACM_OK;
}

int macm_policy_flock_sampled(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows,
                              const macm_sample_config* cfg, uint8_t* actions, float* logits, void* stream) {
  return macm_policy_flock_sampled_at(p, obs, obs_f64, 0, rows, cfg, actions, logits, stream);
}

int macm_value_flock(const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t rows, float* values,
                     void* stream) {
  if (!c) return fail(MACM_E_INVALID, "critic is NULL");
  if (const int rc = mlp_check("critic", c)) return rc;
  if (!obs || !values) return fail(MACM_E_INVALID, "obs/values is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "rows must be >= 0");
  const ValueArgs V{c->params, nullptr, nullptr, c->hidden, c->n_hidden};
  HIP_TRY(launch_value_flock(V, obs, obs_f64 != 0, c->in_dim, rows, values, (hipStream_t)stream));
  return MACM_OK;
}

int macm_gae(const float* reward, const float* values, const float* boot, const uint8_t* done, int32_t n_steps,
             int32_t n_envs, int32_t n_agents, float gamma, float lambda, float* adv, float* ret, void* stream) {
  if (!reward || !values || !boot || !done || !adv || !ret)
    return fail(MACM_E_INVALID, "gae: reward/values/boot/done/adv/ret is NULL");
  if (n_steps < 0 || n_envs < 0 || n_agents < 0) return fail(MACM_E_INVALID, "gae: n_steps, n_envs, n_agents must be >= 0");
  const GaeShape g{n_steps, n_envs, n_agents, gamma, lambda};
  HIP_TRY(launch_gae(reward, values, boot, done, g, adv, ret, (hipStream_t)stream));
  return MACM_OK;
}

// The workspace of macm_policy_grad / macm_value_grad: one partial of the largest net per wave
static int64_t mlp_grad_workspace_bytes(int64_t rows) {
  return (int64_t)mlp_grad_partials(rows) * kGradMaxParams * (int64_t)sizeof(float);
}

int macm_mlp_grad_workspace(int64_t rows, int64_t* bytes) {
  if (!bytes) return fail(MACM_E_INVALID, "grad: bytes is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "grad: rows must be >= 0");
  *bytes = mlp_grad_workspace_bytes(rows);
  return MACM_OK;
}

// A checked policy (n_out = kPolicyLogits) or critic (1) as the gradient launches take it
extern "C++" template <typename M>
static MlpNet net_of(const M* m, int n_out) {
  return MlpNet{m->params, m->in_dim, m->hidden, m->n_hidden, n_out};
}

// What the two gradient calls share behind their struct checks
static int mlp_grad(const MlpNet& net, const void* obs, int32_t obs_f64, int64_t rows, const float* dout, float* grad,
                    void* workspace, int64_t workspace_bytes, void* stream) {
  if (!obs || !dout || !grad) return fail(MACM_E_INVALID, "grad: obs/dout/grad is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "grad: rows must be >= 0");
  if (rows > 0 && !workspace) return fail(MACM_E_INVALID, "grad: workspace is NULL");
  if (rows > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail(MACM_E_INVALID, "grad: workspace must be 16-byte aligned");
  if (rows > 0 && workspace_bytes < mlp_grad_workspace_bytes(rows))
    return fail(MACM_E_INVALID, "grad: workspace_bytes " + std::to_string(workspace_bytes) + " is below the " +
                                    std::to_string(mlp_grad_workspace_bytes(rows)) + " of macm_mlp_grad_workspace");
  HIP_TRY(launch_mlp_grad(net, obs, obs_f64 != 0, rows, dout, grad, (float*)workspace, (hipStream_t)stream));
  return MACM_OK;
}

int macm_policy_grad(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows, const float* dlogits,
                     float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p) return fail(MACM_E_INVALID, "policy is NULL");
  if (const int rc = mlp_check("policy", p)) return rc;
  return mlp_grad(net_of(p, kPolicyLogits), obs, obs_f64, rows, dlogits, grad, workspace, workspace_bytes, stream);
}

int macm_value_grad(const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t rows, const float* dvalues,
                    float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!c) return fail(MACM_E_INVALID, "critic is NULL");
  if (const int rc = mlp_check("critic", c)) return rc;
  return mlp_grad(net_of(c, 1), obs, obs_f64, rows, dvalues, grad, workspace, workspace_bytes, stream);
}

// ---- the PPO loss (ppo_row.hpp): one-shot kernels and loss-to-gradient launches ------------------------
static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
static int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// The workspace of macm_ppo_loss / macm_ppo_grad: the gradient partials, and behind them one stat partial
// per wave (macm_ppo_loss has at most as many blocks as macm_ppo_grad has waves)
static int64_t ppo_stat_offset(int64_t rows) { return align16(mlp_grad_workspace_bytes(rows)); }
static int64_t ppo_workspace_bytes(int64_t rows) {
  return ppo_stat_offset(rows) + (int64_t)mlp_grad_partials(rows) * kPpoStatSlots * (int64_t)sizeof(double);
}

int macm_ppo_workspace(int64_t rows, int64_t* bytes) {
  if (!bytes) return fail(MACM_E_INVALID, "ppo: bytes is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "ppo: rows must be >= 0");
  *bytes = ppo_workspace_bytes(rows);
  return MACM_OK;
}

int macm_policy_logp(const float* logits, const uint8_t* actions, int64_t rows, float* logp, float* entropy,
                     void* stream) {
  if (!logits || !actions || !logp) return fail(MACM_E_INVALID, "logp: logits/actions/logp is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "logp: rows must be >= 0");
  if (misaligned(logits, 4) || misaligned(logp, 4) || misaligned(entropy, 4))
    return fail(MACM_E_INVALID, "logp: logits, logp and entropy must be 4-byte aligned");
  HIP_TRY(launch_policy_logp(logits, actions, rows, logp, entropy, (hipStream_t)stream));
  return MACM_OK;
}

// What macm_ppo_loss and macm_ppo_grad check alike: the config, rows and the workspace
static int ppo_check(const macm_ppo_config* cfg, int64_t rows, bool clipped_value, const double* stats,
                     const void* workspace, int64_t workspace_bytes) {
  if (!cfg) return fail(MACM_E_INVALID, "ppo: cfg is NULL");
  if (!(cfg->clip > 0.0f)) return fail(MACM_E_INVALID, "ppo: clip must be > 0");
  if (!(cfg->vf_coef >= 0.0f) || !(cfg->ent_coef >= 0.0f))
    return fail(MACM_E_INVALID, "ppo: vf_coef and ent_coef must be >= 0");
  if (clipped_value && !(cfg->vf_clip > 0.0f))
    return fail(MACM_E_INVALID, "ppo: vf_clip must be > 0 where old_values is given");
  for (int i = 0; i < 4; ++i)
    if (cfg->reserved[i] != 0) return fail(MACM_E_INVALID, "ppo: reserved must be 0");
  if (rows < 0) return fail(MACM_E_INVALID, "ppo: rows must be >= 0");
  if (misaligned(stats, 8)) return fail(MACM_E_INVALID, "ppo: stats must be 8-byte aligned");
  if (rows > 0 && !workspace) return fail(MACM_E_INVALID, "ppo: workspace is NULL");
  if (rows > 0 && misaligned(workspace, 16)) return fail(MACM_E_INVALID, "ppo: workspace must be 16-byte aligned");
  if (rows > 0 && workspace_bytes < ppo_workspace_bytes(rows))
    return fail(MACM_E_INVALID, "ppo: workspace_bytes " + std::to_string(workspace_bytes) + " is below the " +
                                    std::to_string(ppo_workspace_bytes(rows)) + " of macm_ppo_workspace");
  return MACM_OK;
}

int macm_ppo_loss(const macm_ppo_config* cfg, int64_t rows, const float* logits, const uint8_t* actions,
                  const float* old_logp, const float* adv, const float* values, const float* ret,
                  const float* old_values, const float* scale, float* dlogits, float* dvalues, double* stats,
                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (const int rc = ppo_check(cfg, rows, old_values != nullptr, stats, workspace, workspace_bytes)) return rc;
  if (!logits && !values) return fail(MACM_E_INVALID, "ppo: logits and values are both NULL");
  if (logits && (!actions || !old_logp || !adv))
    return fail(MACM_E_INVALID, "ppo: actions/old_logp/adv is NULL where logits is given");
  if (values && !ret) return fail(MACM_E_INVALID, "ppo: ret is NULL where values is given");
  if (dlogits && !logits) return fail(MACM_E_INVALID, "ppo: dlogits is wanted but logits is NULL");
  if (dvalues && !values) return fail(MACM_E_INVALID, "ppo: dvalues is wanted but values is NULL");
  for (const void* p : {(const void*)logits, (const void*)old_logp, (const void*)adv, (const void*)values,
                        (const void*)ret, (const void*)old_values, (const void*)scale, (const void*)dlogits,
                        (const void*)dvalues})
    if (misaligned(p, 4)) return fail(MACM_E_INVALID, "ppo: the float32 arrays must be 4-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  if (rows == 0) {
    if (stats) HIP_TRY(hipMemsetAsync(stats, 0, 8 * sizeof(double), s));
    return MACM_OK;
  }
  const PpoCfg c{cfg->clip, cfg->vf_coef, cfg->ent_coef, cfg->vf_clip};
  double* const part = stats ? reinterpret_cast<double*>((char*)workspace + ppo_stat_offset(rows)) : nullptr;
  const PpoLossArgs A{logits, actions, old_logp, adv, values, ret, old_values, scale, dlogits, dvalues, part, c};
  HIP_TRY(launch_ppo_loss(A, rows, s));
  if (stats)
    HIP_TRY(launch_ppo_stats(part, (int)ppo_loss_partials(rows), rows, c, logits != nullptr, values != nullptr, stats, s));
  return MACM_OK;
}

// What macm_ppo_grad, macm_ppo_grad_rows and macm_ppo_update refuse alike, before anything is launched
static int ppo_grad_check(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c,
                          const void* obs, int64_t rows, const uint8_t* actions, const float* old_logp,
                          const float* adv, const float* ret, const float* old_values, const float* grad_policy,
                          const float* grad_value, const double* stats, const void* workspace,
                          int64_t workspace_bytes) {
  if (const int rc = ppo_check(cfg, rows, c && old_values, stats, workspace, workspace_bytes)) return rc;
  if (!p && !c) return fail(MACM_E_INVALID, "ppo: policy and critic are both NULL");
  if (p) {
    if (const int rc = mlp_check("policy", p)) return rc;
    if (!actions || !old_logp || !adv || !grad_policy)
      return fail(MACM_E_INVALID, "ppo: actions/old_logp/adv/grad_policy is NULL where the policy is given");
  }
  if (c) {
    if (const int rc = mlp_check("critic", c)) return rc;
    if (!ret || !grad_value) return fail(MACM_E_INVALID, "ppo: ret/grad_value is NULL where the critic is given");
  }
  if (p && c && p->in_dim != c->in_dim)
    return fail(MACM_E_INVALID, "ppo: the policy's in_dim and the critic's differ (they read the same obs rows)");
  if (!obs) return fail(MACM_E_INVALID, "ppo: obs is NULL");
  for (const void* q : {(const void*)old_logp, (const void*)adv, (const void*)ret, (const void*)old_values,
                        (const void*)grad_policy, (const void*)grad_value})
    if (misaligned(q, 4)) return fail(MACM_E_INVALID, "ppo: the float32 arrays must be 4-byte aligned");
  return MACM_OK;
}

// macm_ppo_grad (R NULL) and macm_ppo_grad_rows (R: the index and the advantage's normalisation) behind
// ppo_grad_check: the launches
static int ppo_grad_launch(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c,
                           const void* obs, int32_t obs_f64, int64_t rows, const PpoRowsArgs* R, const uint8_t* actions,
                           const float* old_logp, const float* adv, const float* ret, const float* old_values,
                           float* grad_policy, float* grad_value, double* stats, void* workspace, hipStream_t s) {
  if (rows == 0) {
    if (p) HIP_TRY(hipMemsetAsync(grad_policy, 0, sizeof(float) * net_of(p, kPolicyLogits).n_params(), s));
    if (c) HIP_TRY(hipMemsetAsync(grad_value, 0, sizeof(float) * net_of(c, 1).n_params(), s));
    if (stats) HIP_TRY(hipMemsetAsync(stats, 0, 8 * sizeof(double), s));
    return MACM_OK;
  }
  const PpoCfg k{cfg->clip, cfg->vf_coef, cfg->ent_coef, cfg->vf_clip};
  double* const part = stats ? reinterpret_cast<double*>((char*)workspace + ppo_stat_offset(rows)) : nullptr;
  const PpoGradArgs G{actions, old_logp, adv, ret, c ? old_values : nullptr, k, 1.0 / (double)rows, part};
  const auto launch = [&](const MlpNet& net, float* grad) {
    return R ? launch_mlp_ppo_grad_rows(net, obs, obs_f64 != 0, rows, G, *R, grad, (float*)workspace, s)
             : launch_mlp_ppo_grad(net, obs, obs_f64 != 0, rows, G, grad, (float*)workspace, s);
  };
  if (p) HIP_TRY(launch(net_of(p, kPolicyLogits), grad_policy));
  if (c) HIP_TRY(launch(net_of(c, 1), grad_value));
  if (stats)
    HIP_TRY(launch_ppo_stats(part, (int)mlp_grad_partials(rows), rows, k, p != nullptr, c != nullptr, stats, s));
  return MACM_OK;
}

static int ppo_grad(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs,
                    int32_t obs_f64, int64_t rows, const PpoRowsArgs* R, const uint8_t* actions, const float* old_logp,
                    const float* adv, const float* ret, const float* old_values, float* grad_policy,
                    float* grad_value, double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (const int rc = ppo_grad_check(cfg, p, c, obs, rows, actions, old_logp, adv, ret, old_values, grad_policy,
                                    grad_value, stats, workspace, workspace_bytes))
    return rc;
  return ppo_grad_launch(cfg, p, c, obs, obs_f64, rows, R, actions, old_logp, adv, ret, old_values, grad_policy,
                         grad_value, stats, workspace, (hipStream_t)stream);
}

int macm_ppo_grad(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs,
                  int32_t obs_f64, int64_t rows, const uint8_t* actions, const float* old_logp, const float* adv,
                  const float* ret, const float* old_values, float* grad_policy, float* grad_value, double* stats,
                  void* workspace, int64_t workspace_bytes, void* stream) {
  return ppo_grad(cfg, p, c, obs, obs_f64, rows, nullptr, actions, old_logp, adv, ret, old_values, grad_policy,
                  grad_value, stats, workspace, workspace_bytes, stream);
}

// The source rows of an index: at most what an int32 index can name
static int n_src_check(int64_t n_src) {
  if (n_src < 0 || n_src > (int64_t)INT32_MAX)
    return fail(MACM_E_INVALID, "ppo: n_src must be in [0, 2^31 - 1], got " + std::to_string(n_src));
  return MACM_OK;
}

int macm_ppo_grad_rows(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs,
                       int32_t obs_f64, int64_t rows, const int32_t* index, int64_t n_src, const double* adv_norm,
                       const uint8_t* actions, const float* old_logp, const float* adv, const float* ret,
                       const float* old_values, float* grad_policy, float* grad_value, double* stats, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  if (!index && !adv_norm)
    return fail(MACM_E_INVALID, "ppo: index and adv_norm are both NULL (that call is macm_ppo_grad)");
  if (const int rc = n_src_check(n_src)) return rc;
  if (misaligned(index, 4)) return fail(MACM_E_INVALID, "ppo: index must be 4-byte aligned");
  if (misaligned(adv_norm, 8)) return fail(MACM_E_INVALID, "ppo: adv_norm must be 8-byte aligned");
  const PpoRowsArgs R{index, n_src, adv_norm};
  return ppo_grad(cfg, p, c, obs, obs_f64, rows, &R, actions, old_logp, adv, ret, old_values, grad_policy, grad_value,
                  stats, workspace, workspace_bytes, stream);
}

int macm_adv_moments(const float* x, const int32_t* index, int64_t n_src, int64_t rows, double eps, double* out,
                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !out) return fail(MACM_E_INVALID, "moments: x/out is NULL");
  if (rows < 0) return fail(MACM_E_INVALID, "moments: rows must be >= 0");
  if (const int rc = n_src_check(n_src)) return rc;
  if (!(eps >= 0.0) || std::isinf(eps)) return fail(MACM_E_INVALID, "moments: eps must be finite and >= 0");
  if (misaligned(x, 4) || misaligned(index, 4))
    return fail(MACM_E_INVALID, "moments: x and index must be 4-byte aligned");
  if (misaligned(out, 8)) return fail(MACM_E_INVALID, "moments: out must be 8-byte aligned");
  if (rows > 0 && !workspace) return fail(MACM_E_INVALID, "moments: workspace is NULL");
  if (rows > 0 && misaligned(workspace, 16)) return fail(MACM_E_INVALID, "moments: workspace must be 16-byte aligned");
  if (rows > 0 && workspace_bytes < ppo_workspace_bytes(rows))
    return fail(MACM_E_INVALID, "moments: workspace_bytes " + std::to_string(workspace_bytes) + " is below the " +
                                    std::to_string(ppo_workspace_bytes(rows)) + " of macm_ppo_workspace");
  HIP_TRY(launch_adv_moments(x, index, n_src, rows, eps, out, (double*)workspace, (hipStream_t)stream));
  return MACM_OK;
}

// ---- the PPO update (ppo_adam.hip): the optimiser step, and minibatches enqueued in one call ---------------
static int64_t adam_state_bytes(int n_p, int n_c) {
  return (int64_t)kAdamHead * (int64_t)sizeof(double) + 2 * ((int64_t)n_p + n_c) * (int64_t)sizeof(float);
}

// The nets of a step: both checked, their parameter counts (an absent net: 0)
static int adam_nets(const macm_policy_mlp* p, const macm_value_mlp* c, int* n_p, int* n_c) {
  if (!p && !c) return fail(MACM_E_INVALID, "adam: policy and critic are both NULL");
  if (p)
    if (const int rc = mlp_check("policy", p)) return rc;
  if (c)
    if (const int rc = mlp_check("critic", c)) return rc;
  *n_p = p ? net_of(p, kPolicyLogits).n_params() : 0;
  *n_c = c ? net_of(c, 1).n_params() : 0;
  return MACM_OK;
}

int macm_ppo_adam_state_bytes(const macm_policy_mlp* p, const macm_value_mlp* c, int64_t* bytes) {
  if (!bytes) return fail(MACM_E_INVALID, "adam: bytes is NULL");
  int n_p, n_c;
  if (const int rc = adam_nets(p, c, &n_p, &n_c)) return rc;
  *bytes = adam_state_bytes(n_p, n_c);
  return MACM_OK;
}

// What macm_ppo_adam refuses, and macm_ppo_update with it; has_stats: the step will be given a stats row
static int adam_check(const macm_adam_config* o, const macm_policy_mlp* p, const macm_value_mlp* c,
                      const float* grad_policy, const float* grad_value, bool has_stats, const void* stats,
                      const void* state, int64_t state_bytes) {
  if (!o) return fail(MACM_E_INVALID, "adam: opt is NULL");
  int n_p, n_c;
  if (const int rc = adam_nets(p, c, &n_p, &n_c)) return rc;
  for (int i = 0; i < 4; ++i)
    if (o->reserved[i] != 0) return fail(MACM_E_INVALID, "adam: reserved must be 0");
  if (!(o->lr >= 0.0) || std::isinf(o->lr)) return fail(MACM_E_INVALID, "adam: lr must be finite and >= 0");
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0))
    return fail(MACM_E_INVALID, "adam: beta1 and beta2 must be in [0, 1)");
  if (!(o->eps > 0.0) || std::isinf(o->eps)) return fail(MACM_E_INVALID, "adam: eps must be finite and > 0");
  if (!(o->max_grad_norm >= 0.0) || std::isinf(o->max_grad_norm))
    return fail(MACM_E_INVALID, "adam: max_grad_norm must be finite and >= 0 (0: no clipping)");
  if (!(o->target_kl >= 0.0) || std::isinf(o->target_kl))
    return fail(MACM_E_INVALID, "adam: target_kl must be finite and >= 0 (0: no gate)");
  if (o->target_kl > 0.0 && (!has_stats || !p))
    return fail(MACM_E_INVALID, "adam: target_kl > 0 needs stats and the policy (approx_kl is the policy's)");
  if ((p && !grad_policy) || (c && !grad_value))
    return fail(MACM_E_INVALID, "adam: grad_policy/grad_value is NULL for a net that is given");
  if (!state) return fail(MACM_E_INVALID, "adam: state is NULL");
  if (misaligned(grad_policy, 4) || misaligned(grad_value, 4))
    return fail(MACM_E_INVALID, "adam: the gradients must be 4-byte aligned");
  if (misaligned(stats, 8)) return fail(MACM_E_INVALID, "adam: stats must be 8-byte aligned");
  if (misaligned(state, 8)) return fail(MACM_E_INVALID, "adam: state must be 8-byte aligned");
  if (state_bytes < adam_state_bytes(n_p, n_c))
    return fail(MACM_E_INVALID, "adam: state_bytes " + std::to_string(state_bytes) + " is below the " +
                                    std::to_string(adam_state_bytes(n_p, n_c)) + " of macm_ppo_adam_state_bytes");
  return MACM_OK;
}

// The step's arguments behind adam_check: the state's layout is the header's
static AdamArgs adam_args(const macm_adam_config* o, const macm_policy_mlp* p, const macm_value_mlp* c,
                          const float* grad_policy, const float* grad_value, const double* stats, void* state) {
  const int n_p = p ? net_of(p, kPolicyLogits).n_params() : 0, n_c = c ? net_of(c, 1).n_params() : 0;
  double* const head = (double*)state;
  float* const mp = (float*)(head + kAdamHead);
  float* const mc = mp + 2 * n_p;
  AdamArgs A;
  A.param[0] = p ? const_cast<float*>(p->params) : nullptr;  // (the structs declare what the forward reads; the step writes it)
  A.param[1] = c ? const_cast<float*>(c->params) : nullptr;
  A.grad[0] = grad_policy;
  A.grad[1] = grad_value;
  A.m[0] = mp;
  A.v[0] = mp + n_p;
  A.m[1] = mc;
  A.v[1] = mc + n_c;
  A.n[0] = n_p;
  A.n[1] = n_c;
  A.head = head;
  A.stats = stats;
  A.lr = o->lr;
  A.beta1 = o->beta1;
  A.beta2 = o->beta2;
  A.omb1 = 1.0 - o->beta1;
  A.omb2 = 1.0 - o->beta2;
  A.eps = o->eps;
  A.max_grad_norm = o->max_grad_norm;
  A.target_kl = o->target_kl;
  return A;
}

int macm_ppo_adam(const macm_adam_config* opt, const macm_policy_mlp* p, const macm_value_mlp* c,
                  const float* grad_policy, const float* grad_value, const double* stats, void* state,
                  int64_t state_bytes, void* stream) {
  if (const int rc = adam_check(opt, p, c, grad_policy, grad_value, stats != nullptr, stats, state, state_bytes))
    return rc;
  HIP_TRY(launch_ppo_adam(adam_args(opt, p, c, grad_policy, grad_value, stats, state), (hipStream_t)stream));
  return MACM_OK;
}

// The workspace of macm_ppo_update: macm_ppo_workspace(max_rows) (the moments' partials, then the gradient and
// stat partials: the launches are ordered), and behind it the moments, a stats row and both gradients
static int64_t update_fixed_bytes() {
  return align16((4 + 8) * (int64_t)sizeof(double) + 2 * (int64_t)kGradMaxParams * (int64_t)sizeof(float));
}

int macm_ppo_update_workspace(int64_t max_rows, int64_t* bytes) {
  if (!bytes) return fail(MACM_E_INVALID, "update: bytes is NULL");
  if (max_rows < 0) return fail(MACM_E_INVALID, "update: max_rows must be >= 0");
  *bytes = ppo_workspace_bytes(max_rows) + update_fixed_bytes();
  return MACM_OK;
}

int macm_ppo_update(const macm_ppo_config* cfg, const macm_adam_config* opt, const macm_policy_mlp* p,
                    const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t n_src, const uint8_t* actions,
                    const float* old_logp, const float* adv, const float* ret, const float* old_values,
                    int32_t n_minibatches, const int32_t* const* index, const int64_t* rows, int32_t normalize_adv,
                    double adv_eps, void* state, int64_t state_bytes, double* stats, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  if (n_minibatches < 0) return fail(MACM_E_INVALID, "update: n_minibatches must be >= 0");
  if (n_minibatches > 0 && (!index || !rows)) return fail(MACM_E_INVALID, "update: index/rows is NULL");
  int64_t max_rows = 0;
  for (int i = 0; i < n_minibatches; ++i) {
    if (rows[i] < 0) return fail(MACM_E_INVALID, "update: rows[" + std::to_string(i) + "] must be >= 0");
    if (rows[i] > 0 && !index[i]) return fail(MACM_E_INVALID, "update: index[" + std::to_string(i) + "] is NULL");
    if (rows[i] > 0 && misaligned(index[i], 4))
      return fail(MACM_E_INVALID, "update: index[" + std::to_string(i) + "] must be 4-byte aligned");
    max_rows = std::max(max_rows, rows[i]);
  }
  if (const int rc = n_src_check(n_src)) return rc;
  if (!(adv_eps >= 0.0) || std::isinf(adv_eps)) return fail(MACM_E_INVALID, "update: adv_eps must be finite and >= 0");
  if (!workspace) return fail(MACM_E_INVALID, "update: workspace is NULL");
  if (misaligned(workspace, 16)) return fail(MACM_E_INVALID, "update: workspace must be 16-byte aligned");
  const int64_t need = ppo_workspace_bytes(max_rows) + update_fixed_bytes();
  if (workspace_bytes < need)
    return fail(MACM_E_INVALID, "update: workspace_bytes " + std::to_string(workspace_bytes) + " is below the " +
                                    std::to_string(need) + " of macm_ppo_update_workspace");
  char* const fixed = (char*)workspace + ppo_workspace_bytes(max_rows);
  double* const norm = (double*)fixed;
  double* const stat1 = norm + 4;
  float* const gp = (float*)(stat1 + 8);
  float* const gv = gp + kGradMaxParams;
  if (const int rc = ppo_grad_check(cfg, p, c, obs, max_rows, actions, old_logp, adv, ret, old_values, gp, gv, stats,
                                    workspace, workspace_bytes))
    return rc;
  if (const int rc = adam_check(opt, p, c, gp, gv, true, stats, state, state_bytes)) return rc;
  const hipStream_t s = (hipStream_t)stream;
  const bool moments = normalize_adv != 0 && p != nullptr;
  for (int i = 0; i < n_minibatches; ++i) {
    double* const st = stats ? stats + (size_t)i * 8 : stat1;
    if (rows[i] == 0) {
      if (stats) HIP_TRY(hipMemsetAsync(st, 0, 8 * sizeof(double), s));
      continue;
    }
    if (moments) HIP_TRY(launch_adv_moments(adv, index[i], n_src, rows[i], adv_eps, norm, (double*)workspace, s));
    const PpoRowsArgs R{index[i], n_src, moments ? norm : nullptr};
    if (const int rc = ppo_grad_launch(cfg, p, c, obs, obs_f64, rows[i], &R, actions, old_logp, adv, ret, old_values,
                                       gp, gv, st, workspace, s))
      return rc;
    HIP_TRY(launch_ppo_adam(adam_args(opt, p, c, gp, gv, st, state), s));
  }
  return MACM_OK;
}

// ============================ scripted actors ===============================

int macm_bots_flock(const void* obs, int32_t obs_f64, int32_t obs_dim, int64_t rows, uint8_t* actions,
                    void* stream) {
  if (!obs || !actions || rows < 0) return fail(MACM_E_INVALID, "obs/actions NULL or rows < 0");
  if (obs_dim != 4 && obs_dim != 6) return fail(MACM_E_INVALID, "obs_dim must be 4 (polar) or 6 (cartesian)");
  HIP_TRY(launch_bots_flock(obs, obs_f64 != 0, obs_dim, rows, actions, (hipStream_t)stream));
  return MACM_OK;
}

int macm_bots_combat(const void* obs, const uint8_t* mask, int32_t obs_f64, int32_t n_agents, int64_t rows,
                     uint8_t* actions, void* stream) {
  if (!obs || !mask || !actions || rows < 0) return fail(MACM_E_INVALID, "obs/mask/actions NULL or rows < 0");
  if (n_agents < 2) return fail(MACM_E_INVALID, "n_agents must be >= 2");
  HIP_TRY(launch_bots_combat(obs, mask, obs_f64 != 0, n_agents, rows, actions, (hipStream_t)stream));
  return MACM_OK;
}

}  // extern "C"
