// This file is the body of the workgroup TDM step kernel, included by tdm_step_wg.hip once per kernel:
//   MACM_TDM_STEP_WG     the kernel's name
//   MACM_TDM_STEP_WG_EV  0: tdm_step_wg; 1: tdm_step_ev_wg, the step of worlds with events registered
//                        (macm_tdm_set_events), which takes hit_out and stores hit_out[e, i] = the body
//                        agent i's attack damaged in this step, or -1, with the committed combat state
// Two texts of one kernel, not a shared function: built from a function the kernel without events
// got other code than it had (its kernarg loads and register allocation), and that kernel is to stay,
// instruction for instruction, what worlds without events have always launched.
// BPT bodies per thread (round 5: N up to 4096 with 1024 threads; thread t holds t, t + BS, ...); BPT = 1
// with blockDim = N rounded up to 64 below 1024 agents. Every ordered step (the listener and damage in
// agent order on thread 0, the spill step's scans) sees the bodies in agent order either way.
template <typename OT, int BPT = 1>
__global__ __launch_bounds__(1024) void MACM_TDM_STEP_WG(StepParams P, WorldBuffers B, TdmParams TP, TdmBuffers TB,
                                                         int cur, const uchar4* __restrict__ actions,
                                                         OT* __restrict__ obs, uint8_t* __restrict__ done_out
#if MACM_TDM_STEP_WG_EV
                                                         ,
                                                         int32_t* __restrict__ hit_out
#endif
) {
  using namespace tdmwg;
  extern __shared__ __align__(16) unsigned char lds[];
  const int e = blockIdx.x, tid = threadIdx.x, BS = blockDim.x, N = P.n_agents;
  const PreLayout L = pre_layout(N);
  float2* s_c = (float2*)(lds + L.c);
  double* s_hpd = (double*)(lds + L.hp);
  int* s_hit = (int*)(lds + L.hit);
  uint32_t* s_aw = (uint32_t*)(lds + L.aw);
  uint32_t* s_atw = (uint32_t*)(lds + L.atw);

  // The spill working-set slot is taken before anything of this step is committed: a pool that
  // stays full (~1 s) leaves the env wholly unstepped and reported, never half-stepped (ADVICE r03)
  __shared__ int s_slot;
  const int slot = spill::acquire_slot(B, e, &s_slot);
  if (slot < 0) {
    spill::keep_lists(P, B, e, cur);
    if (tid == 0) {
      B.status[e] |= MACM_ST_SPILL_WAIT;
      report_status(B, MACM_ST_SPILL_WAIT);
    }
    return;
  }
  bool act[BPT], act0[BPT], attacking[BPT];
  float2 p[BPT], F[BPT];
  float ang[BPT], ray_x[BPT], ray_y[BPT];
  double hp[BPT], cda[BPT], cdm[BPT];  // Agent.health, cooldown_atk, cooldown_mov_penalty
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int i = tid + j * BS;
    const size_t ag = (size_t)e * N + i;
    act[j] = false;
    p[j] = F[j] = make_float2(0.0f, 0.0f);
    ang[j] = ray_x[j] = ray_y[j] = 0.0f;
    hp[j] = cda[j] = cdm[j] = 0.0;
    attacking[j] = false;
    int a0 = 1, a1 = 1, a2 = 1, a3 = 0;
    if (i < N) {
      p[j] = B.pos[ag];
      ang[j] = B.angle[ag];
      const uchar4 a = actions[ag];
      a0 = a.x;
      a1 = a.y;
      a2 = a.z;
      a3 = a.w;
      act[j] = TB.alive[ag] != 0;
      hp[j] = TB.health[ag];
      cda[j] = TB.cd_atk[ag];
      cdm[j] = TB.cd_mov[ag];
      s_c[i] = p[j];
      s_hpd[i] = hp[j];
    }
    act0[j] = act[j];  // alive when the step starts (acts this step)

    // ---- the action loop (combat.py:121-155), as env_step_w64<kTdm> ------------------------------
    if (act[j]) {
      // agent.body.angle = angle + (a2-1) * rotation_speed * (1/hz) -> SetTransform(float32)
      float af = (float)((double)ang[j] + ((double)(a2 - 1) * P.rot_step) * P.inv_hz);
      const double ad = (double)af;
      if (fabs(ad) > M_PI) af = (float)(ad - sgn(ad) * (2.0 * M_PI));
      ang[j] = af;
      const double cc = ((a0 != 1) && (a1 != 1)) ? P.diag_c : 1.0;
      const double k0 = (double)(a0 - 1), k1 = (double)(a1 - 1);
      // Agent.force = _force * (1 - percent_mov_penalty * int(cooldown_mov_penalty > 0))   combat.py:46-49
      const double force = P.force * (1.0 - TP.percent_mov_penalty * (double)(cdm[j] > 0.0));
      double s0, c0, s1, c1;  // np.cos / np.sin of angle and angle + pi/2
      act_trig(af, &s0, &c0, &s1, &c1);
      F[j].x = 0.0f + (float)((c0 * k0 + c1 * k1) * cc * force);  // ApplyForce onto ClearForces' zero
      F[j].y = 0.0f + (float)((s0 * k0 + s1 * k1) * cc * force);
      if (cda[j] <= 0.0) {
        if (a3) {
          attacking[j] = true;
          // point2 = point1 + (range*cos(angle), range*sin(angle)): a float32 add of the
          // float32-converted tuple
          ray_x[j] = p[j].x + (float)(TP.melee_range * c0);
          ray_y[j] = p[j].y + (float)(TP.melee_range * s0);
          cda[j] = TP.cooldown_atk;
          cdm[j] = TP.cooldown_mov_penalty;
        }
      } else {
        cda[j] -= P.inv_hz;
        if (TP.decay_mov_penalty) cdm[j] -= P.inv_hz;
      }
    }
    ballot_bits(s_aw, N, act[j], j);
    ballot_bits(s_atw, N, attacking[j], j);
  }
  __syncthreads();  // positions, health and both bitmaps visible

  // ---- ray casts: b2World::RayCast + RayCastClosestCallback (cm_framework.py:56-86) --------------
#pragma unroll
  for (int jj = 0; jj < BPT; ++jj) {
    if (!attacking[jj]) continue;
    int hit = -1;
    const float rvx = ray_x[jj] - p[jj].x, rvy = ray_y[jj] - p[jj].y;  // r = p2 - p1
    const float rrr = rvx * rvx + rvy * rvy;
    const float rad2 = P.radius * P.radius;
    float maxf = 1.0f;
    for (int q = 0; q < words(N); ++q)
      for (uint32_t m = s_aw[q]; m; m &= m - 1u) {
        const int j = 32 * q + __builtin_ctz(m);
        const float2 cj = s_c[j];
        const float sx = p[jj].x - cj.x, sy = p[jj].y - cj.y;  // s = p1 - position
        const float bb = (sx * sx + sy * sy) - rad2;
        const float c = sx * rvx + sy * rvy;
        const float sigma = c * c - rrr * bb;
        if (sigma < 0.0f || rrr < kEps) continue;
        float a = -(c + sqrtf(sigma));
        if (0.0f <= a && a <= maxf * rrr) {
          a /= rrr;
          maxf = a;
          hit = j;
        }
      }
    s_hit[tid + jj * BS] = hit;
  }
  __syncthreads();
  int2 lis = make_int2(0, -1);
  if (tid == 0) {
    // listener.hit / listener.fixture persist across casts and steps (literal), or reset per cast
    // (fresh_raycast); damage in agent order (combat.py:152-153)
    lis = TB.listener[e];
    for (int q = 0; q < words(N); ++q)
      for (uint32_t m = s_atw[q]; m; m &= m - 1u) {
        const int k = 32 * q + __builtin_ctz(m);
        const int h = s_hit[k];
        if (TP.fresh_raycast) {
          if (h >= 0) s_hpd[h] -= TP.melee_dmg;
        } else {
          if (h >= 0) lis = make_int2(1, h);
          if (lis.x) s_hpd[lis.y] -= TP.melee_dmg;
#if MACM_TDM_STEP_WG_EV
          // the damaged body, the listener's after this cast, back into the attacker's entry
          // (fresh_raycast: the entry already is it)
          s_hit[k] = lis.x ? lis.y : -1;
#endif
        }
      }
  }
  __syncthreads();
  int n_alive0 = 0, n_att = 0, n_died = 0;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int i = tid + j * BS;
    if (i < N) hp[j] = s_hpd[i];
    if (act[j] && hp[j] <= 0.0) act[j] = false;  // deaths: body.active = False (combat.py:157-165)
    n_alive0 += __syncthreads_count(act0[j]);
    n_att += __syncthreads_count(attacking[j]);
    n_died += __syncthreads_count(act0[j] && !act[j]);
  }

  // ---- commit the combat state (the spill step reads it back) ------------------------------------
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int i = tid + j * BS;
    const size_t ag = (size_t)e * N + i;
    if (i < N) {
      if (act0[j]) {
        B.angle[ag] = ang[j];
        TB.cd_atk[ag] = cda[j];
        TB.cd_mov[ag] = cdm[j];
      }
      TB.health[ag] = hp[j];
      TB.alive[ag] = act[j] ? 1 : 0;
      if (TB.health_out) TB.health_out[ag] = hp[j];
      if (TB.alive_out) TB.alive_out[ag] = act[j] ? 1 : 0;
#if MACM_TDM_STEP_WG_EV
      // only attackers' entries of s_hit were written; thread 0's updates are behind the barrier above
      hit_out[ag] = attacking[j] ? s_hit[i] : -1;
#endif
    }
  }
  if (tid == 0) {
    TB.listener[e] = lis;
    unsigned long long* ec = B.env_counters + (size_t)e * 4;
    ec[0] += (unsigned long long)n_alive0;
    ec[1] += (unsigned long long)n_att;
    ec[2] += (unsigned long long)n_died;
  }
  __threadfence_block();
  // ---- Box2D step of the living bodies, TDM.get_obs, done / winner --------------------------------
  // (above 1024 agents the pair records live in the slot's HBM: 48 B per body would not fit beside
  // the per-body arrays)
  spill::step_env<OT, BPT == 1, kTdm, BPT, true>(P, B, e, cur, actions, obs, nullptr, nullptr, nullptr, done_out, lds, &TP,
                                           &TB, F, slot);
}
