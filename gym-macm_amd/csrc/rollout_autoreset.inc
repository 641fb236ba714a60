// rollout_autoreset.inc — the multi-step wave kernels of a world with autoreset on
// (macm_world_set_autoreset / macm_tdm_set_autoreset): env_rollout_w64's loop with the episode
// restart inside it. Included by flock_step_w64.hip in the translation unit flock_rollout_ar_w64.hip
// only, so the kernels of worlds without autoreset stay the objects they were.
//
// An env whose step k sets `done` is reset by its own wave before step k + 1, exactly as
// macm_*_reset_envs would with that step's done flags as the mask:
//   draw_poses_wave : the env's CPython MT19937 stream (env_reset.hip: [E][kMtStride] words in HBM)
//                     continued by one wave: state into LDS, one twist at most (6 N <= 384 words a
//                     reset), 6 N tempered words, random() = res53 and the pose formulas of
//                     draw_poses_kernel in the same exactly rounded double arithmetic, state back;
//   *_init_env      : the bodies of the init kernels (flock_init_w64 / tdm_init_w64): zero dynamics,
//                     fresh fat AABBs, the first FindNewContacts list into the buffer the next step
//                     reads, the bookkeeping cleared, and the new episode's initial observation
//                     into step k's output row (obs, nbr_id / mask). The terminal values of step k
//                     (done, reward, collided; TDM winner, health, alive) stay as the step wrote them.
// Every LDS array of the step is dead between two steps: the MT state, the drawn words and TDM
// init's pose arrays (ResetLds) lie over the step's contact pool, so the kernels' LDS is the
// step's. After a reset the next step loads from global memory behind the workgroup fence (the
// carried Flock step: StepCarry::valid = false, which discards the carried next-step actions too).

constexpr int kMtN = 624, kMtM = 397;

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

__device__ __forceinline__ uint32_t mt_mix(uint32_t hi, uint32_t lo, uint32_t src) {
  const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
  return src ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

struct ResetLds {
  uint32_t mt[kMtN];  // 2,496 B
  uint32_t w[6 * W];  // 1,536 B: three random() of two words per agent
  float2 p[W];        // TDM init's poses (tdm_init_env)
  float a[W];
};

// One MT19937 twist of s_mt in place by one wave: the four phases of mt_twist (env_reset.hip), each
// reading only values final for it, with the wave's in-order LDS accesses in place of the block
// barrier (wave_lds_sync). ceil(227 / 64) = 4 values per lane and phase.
__device__ __forceinline__ void mt_twist_wave(uint32_t* s_mt, int lane) {
  const int lo[4] = {0, kMtN - kMtM, 2 * (kMtN - kMtM), kMtN - 1};
  const int hi[4] = {kMtN - kMtM, 2 * (kMtN - kMtM), kMtN - 1, kMtN};
  for (int ph = 0; ph < 4; ++ph) {
    uint32_t v[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int k = lo[ph] + lane + n * W;
      v[n] = 0u;
      if (k < hi[ph]) {
        const int src = k + kMtM < kMtN ? k + kMtM : k + kMtM - kMtN;
        v[n] = mt_mix(s_mt[k], s_mt[k + 1 < kMtN ? k + 1 : 0], s_mt[src]);
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int k = lo[ph] + lane + n * W;
      if (k < hi[ph]) s_mt[k] = v[n];
    }
    wave_lds_sync();
  }
}

// The next 3 N random() of env stream g as the poses of the env's N <= 64 agents (lane = agent),
// stored to pos / angle rows ag; the stream's state and position go back to g.
template <int MODE>
__device__ __forceinline__ void draw_poses_wave(uint32_t* __restrict__ g, const PoseDraw& D, ResetLds* L, int N,
                                                int lane, size_t ag, float2* __restrict__ pos,
                                                float* __restrict__ angle) {
  for (int k = lane; k < kMtN; k += W) L->mt[k] = g[k];
  int idx = __builtin_amdgcn_readfirstlane((int)g[kMtN]);
  wave_lds_sync();
  const int need = 6 * N;
  for (int got = 0; got < need;) {
    if (idx >= kMtN) {
      mt_twist_wave(L->mt, lane);
      idx = 0;
    }
    const int take = min(kMtN - idx, need - got);
    for (int w = lane; w < take; w += W) L->w[got + w] = mt_temper(L->mt[idx + w]);
    got += take;
    idx += take;
    wave_lds_sync();
  }
  if (lane < N) {
    double r[3];
    for (int q = 0; q < 3; ++q) {  // random.random(): genrand_res53
      const uint32_t a = L->w[6 * lane + 2 * q] >> 5, b = L->w[6 * lane + 2 * q + 1] >> 6;
      r[q] = (a * 67108864.0 + b) * (1.0 / 9007199254740992.0);
    }
    double x, y;
    if constexpr (MODE == kFlock) {  // mvmnt.py:62-63
      x = D.spread * (r[0] - 0.5) + D.start_x;
      y = D.spread * (r[1] - 0.5) + D.start_y;
    } else {  // combat.py:83-84
      x = r[0] * ((double)tdm_team_of(D.TP, lane) + D.half_width);
      y = r[1] * D.height;
    }
    const double a = (-1.0 + (1.0 - -1.0) * r[2]) * M_PI;  // random.uniform(-1, 1) * np.pi
    pos[ag] = make_float2((float)x, (float)y);
    angle[ag] = (float)a;
  }
  for (int k = lane; k < kMtN; k += W) g[k] = L->mt[k];
  if (lane == 0) g[kMtN] = (uint32_t)idx;
}

// macm_*_reset_envs of env e by its own wave between two steps of a rollout. `cur` is the list
// buffer the next step reads; obs / nbr_out / TB.mask_out are step k's output rows. The init body
// reads the poses back from the rows this lane just stored (a lane's accesses to one address stay
// in order). TDM: the terminal health / alive / winner outputs are kept (the init kernel would
// overwrite them).
template <int MODE, typename OT>
__device__ __forceinline__ void reset_env_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                              TdmBuffers TB, const PoseDraw& D, uint32_t* __restrict__ mt, int cur,
                                              OT* __restrict__ obs, int32_t* __restrict__ nbr_out, int e, int lane,
                                              void* lds) {
  ResetLds* const L = static_cast<ResetLds*>(lds);
  const size_t ag = (size_t)e * P.n_agents + lane;
  draw_poses_wave<MODE>(mt + (size_t)e * kMtStride, D, L, P.n_agents, lane, ag, B.pos, B.angle);
  if constexpr (MODE == kTdm) {
    TB.health_out = nullptr;
    TB.alive_out = nullptr;
    TB.winner_out = nullptr;
    tdm_init_env<OT>(P, B, TP, TB, cur, obs, e, lane, L->p, L->a);
  } else {
    flock_init_env<OT>(P, B, cur, obs, nbr_out, e, lane);
  }
}

// What the reset is about to overwrite, kept in the env's row of the registered final outputs
// (macm_*_set_final_outputs), by the env's own wave behind the fence that follows the step: obs /
// nbr_out / mask_out are step k's output rows as the step stored them. Flock: lane = agent copies the
// row it stored itself (a float32 polar row is one 16-byte vector). TDM: the env's N (N - 1) slots are
// contiguous and 16-byte aligned, copied lane-strided as 16-byte vectors (a float64 slot: two); its
// N (N - 1) mask bytes by bytes (20 * 19 = 380: a mask row is not 16-byte aligned in general).
// length is the step count the step wrote back (an episode-ending step always does: wb), by the lane
// that stored it. Nothing registered: one wave-uniform test.
template <int MODE, typename OT>
__device__ __forceinline__ void final_copy_w64(const FinalOut& F, const WorldBuffers& B, int N, int od,
                                               const OT* __restrict__ obs, const int32_t* __restrict__ nbr_out,
                                               const uint8_t* __restrict__ mask_out, int e, int lane) {
  if (!F.any()) return;
  if constexpr (MODE == kFlock) {
    if (lane < N) {
      const size_t ag = (size_t)e * N + lane;
      if (F.obs) {
        OT* const dst = static_cast<OT*>(F.obs) + ag * od;
        const OT* const src = obs + ag * od;
        if (sizeof(OT) == 4 && od == 4) {
          *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
        } else {
          for (int q = 0; q < od; ++q) dst[q] = src[q];
        }
      }
      if (F.nbr_id) F.nbr_id[ag] = nbr_out[ag];
    }
  } else {
    const size_t S = (size_t)N * (N - 1);  // the env's slots
    if (F.obs) {
      const size_t nv = S * (sizeof(OT) / 4);  // 16-byte vectors
      const uint4* const src = reinterpret_cast<const uint4*>(obs + (size_t)e * S * 4);
      uint4* const dst = reinterpret_cast<uint4*>(static_cast<OT*>(F.obs) + (size_t)e * S * 4);
      for (size_t v = lane; v < nv; v += W) dst[v] = src[v];
    }
    if (F.mask) {
      const uint8_t* const src = mask_out + (size_t)e * S;
      uint8_t* const dst = F.mask + (size_t)e * S;
      for (size_t b = lane; b < S; b += W) dst[b] = src[b];
    }
  }
  if (lane == 0) {
    if (F.length) F.length[e] = B.step_count[e];
    if (F.ends) F.ends[e] += 1;
  }
}

template <typename OT>
struct RolloutArArgs {  // the kernel's only argument (kernarg offset 0)
  RolloutArgs<OT> A;
  uint32_t* mt;  // [E][kMtStride] the envs' streams
  PoseDraw D;
  FinalOut F;  // last: the fields before it keep their offsets
};
// worlds with events registered (ObsEv, flock_step_w64.hip): A is the plain RolloutArgs still, so the
// fields above keep their offsets, and the event pointer follows them
template <typename OT>
struct RolloutArArgs<ObsEv<OT>> : RolloutArArgs<OT> {
  int32_t* hit_out;  // [E, N], or [K, E, N] with A.traj
};

// a registered policy (ObsPol): likewise, the policy's fields follow
template <typename OT>
struct RolloutArArgs<ObsPol<OT>> : RolloutArArgs<OT> {
  PolicyArgs pol;  // noise [K, E, N, 9], logits [E, N, 9] or [K, E, N, 9] with A.traj
};

// a registered critic beside the policy (ObsPolV): its fields follow the policy's
template <typename OT>
struct RolloutArArgs<ObsPolV<OT>> : RolloutArArgs<ObsPol<OT>> {
  ValueArgs val;  // values [E, N] or [K + 1, E, N], boot [E, N] or [K, E, N] with A.traj
};

// a world with sampling on (ObsPolS / ObsPolVS): the draw's seed, first decision and first row follow
template <typename OT>
struct RolloutArArgs<ObsPolS<OT>> : RolloutArArgs<ObsPol<OT>> {
  SampleArgs smp;  // the decision after step k draws at smp.decision + k (pol.noise is not read)
};
template <typename OT>
struct RolloutArArgs<ObsPolVS<OT>> : RolloutArArgs<ObsPolV<OT>> {
  SampleArgs smp;
};
// a TDM world under a registered set policy (ObsTdmPol / ObsTdmPolEv): the policy's fields follow
template <typename OT>
struct RolloutArArgs<ObsTdmPol<OT>> : RolloutArArgs<OT> {
  TdmPolicyArgs tpol;  // noise [K, E, N, 11], logits [E, N, 11] or [K, E, N, 11] with A.traj
};
template <typename OT>
struct RolloutArArgs<ObsTdmPolEv<OT>> : RolloutArArgs<ObsEv<OT>> {
  TdmPolicyArgs tpol;
};

// env_rollout_w64 with the in-launch reset; no tail or split observation (their pose snapshots know
// nothing of a mid-launch respawn: TDM observes inside the step).
// OTA: OT or ObsEv<OT>, as env_rollout_w64. The step writes the events, the in-launch reset none: it
// gets no pointer to them, as it gets no health_out.
template <int MODE, int NCAP, typename OTA, bool SCAL = false, bool CARRY = false>
__global__ __launch_bounds__(W) __attribute__((amdgpu_waves_per_eu(4))) void env_rollout_ar_w64(RolloutArArgs<OTA> R0) {
  using OT = typename ObsTag<OTA>::type;
  constexpr bool EV = ObsTag<OTA>::ev;
  constexpr bool POL = ObsTag<OTA>::pol;
  constexpr bool VAL = ObsTag<OTA>::val;
  constexpr bool SMP = ObsTag<OTA>::smp;
  constexpr bool TPOL = ObsTag<OTA>::tpol;
  static_assert(!EV || MODE == kTdm, "combat events are TDM's");
  static_assert(!POL || (MODE == kFlock && !CARRY), "the MLP policy acts in Flock's closed loop");
  static_assert(!TPOL || (MODE == kTdm && !CARRY), "the set policy acts in TDM's closed loop");
  const int nsteps = R0.A.nsteps;
  const bool bal = R0.A.B.sched && nsteps >= kRollBalanceMinSteps;  // as in launch_roll_ar
  const int env = bal ? (int)R0.A.B.sched[R0.A.sched_off + blockIdx.x] : (int)blockIdx.x;
  StepCarry cy{};  // CARRY; not valid: the first step loads
  // the candidate lists of the nearest-neighbour sweep (near_build); an in-launch reset clears them
  constexpr bool kNearL = MODE == kFlock && NCAP == 64;
  int near_keep = 0;
  for (int k = 0; k < nsteps; ++k) {
    // as env_rollout_w64: the arguments afresh every step, through a pointer the compiler cannot see through
    const __attribute__((address_space(4))) RolloutArArgs<OTA>* ka =
        (const __attribute__((address_space(4))) RolloutArArgs<OTA>*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const RolloutArArgs<OTA>& R = *(const RolloutArArgs<OTA>*)ka;
    const RolloutArgs<OT>& A = R.A;
    const int N = A.P.n_agents, lane = threadIdx.x;
    const size_t EN = (size_t)A.P.n_envs * N;
    const size_t kr = A.traj ? (size_t)k : 0;  // output row of this step
    const size_t od = MODE == kTdm ? (size_t)(N - 1) * 4 : (A.P.coord == MACM_COORD_CARTESIAN ? 6 : 4);
    OT* const obs = traj_row(A.obs, kr, EN * od);
    int32_t* const nbr = traj_row(A.nbr_out, kr, EN);
    TdmBuffers TB = A.TB;
    if constexpr (MODE == kTdm) {
      TB.mask_out = traj_row(TB.mask_out, kr, EN * (N - 1));
      TB.health_out = traj_row(TB.health_out, kr, EN);
      TB.alive_out = traj_row(TB.alive_out, kr, EN);
      TB.winner_out = traj_row(TB.winner_out, kr, (size_t)A.P.n_envs);
    }
    int32_t* hit_out = nullptr;
    if constexpr (EV) hit_out = R.hit_out + kr * EN;
    const size_t abytes = MODE == kTdm ? 4 : 3;  // closed loop: uint8 actions per agent
    uint8_t* const pol_in = A.policy_act ? A.policy_act + kr * EN * abytes : nullptr;
    __builtin_amdgcn_s_setprio(0);  // as at a launch: the chain raises it again
    // (with the critic as well: the step's lane-derived addresses held across all K steps beside the
    // critic's registers cost the N = 64 kernels a VGPR in scratch. Masked back to its range there:
    // the helpers the Flock kernels share are specialised on the range of the lane they are called with,
    // and an unbounded one here changed the code of every other Flock kernel of the unit.)
    int sl = (int)threadIdx.x;
    if constexpr (MODE == kTdm || VAL) asm volatile("" : "+v"(sl));
    if constexpr (VAL) sl &= W - 1;
    void* lds = nullptr;  // the step's contact pool, dead once the step ends
    const int near_ctl = (kNearL ? near_keep | ((A.cur & kRollNearPlainBit) ? kNearCtlPlain : 0) : 0) |
                         (CARRY && (A.cur & kRollReloadBit) ? kStepCtlWriteBack : 0);
    if constexpr (CARRY) {
      const unsigned char* const act_k = static_cast<const unsigned char*>(A.actions) + (size_t)k * A.astride;
      step_w64_body<MODE, NCAP, OT, SCAL, true, kNearL>(
          A.P, A.B, A.TP, TB, (A.cur ^ k) & 1, act_k, obs, nbr, traj_row(A.rew_out, kr, EN), traj_row(A.coll_out, kr, EN),
          traj_row(A.done_out, kr, (size_t)A.P.n_envs), env, sl, nullptr, &cy,
          k + 1 < nsteps ? act_k + A.astride : nullptr, &lds, near_ctl);
    } else {
      step_w64_body<MODE, NCAP, OT, SCAL, false, kNearL, EV>(
          A.P, A.B, A.TP, TB, kNearL ? (A.cur ^ k) & 1 : A.cur ^ (k & 1),
          pol_in ? pol_in : static_cast<const unsigned char*>(A.actions) + (size_t)k * A.astride, obs, nbr,
          traj_row(A.rew_out, kr, EN), traj_row(A.coll_out, kr, EN), traj_row(A.done_out, kr, (size_t)A.P.n_envs), env, sl,
          nullptr, nullptr, nullptr, &lds, near_ctl, hit_out);
    }
    // the step's done flag, wave-uniform once broadcast from lane 0, which stored it (a lane's
    // accesses to one address stay in order)
    // (TDM: the lane index opaque once more, or what the reset derives from it is computed before
    // the step and held across it: 5 VGPRs in scratch)
    int rl = (int)threadIdx.x;
    if constexpr (MODE == kTdm || VAL) asm volatile("" : "+v"(rl));
    if constexpr (VAL) rl &= W - 1;
    int dn = 0;
    if (rl == 0) dn = A.B.done[env];
    dn = __builtin_amdgcn_readfirstlane(dn);
    if constexpr (kNearL) near_keep = dn ? 0 : kNearCtlKeep;
    if constexpr (CARRY) {
      if (dn || (A.cur & kRollReloadBit)) cy.valid = false;
      if (!cy.valid) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    } else {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    __syncthreads();
    if constexpr (VAL) {
      // The critic around the reset, one copy of its code: pass 0 on the obs row the step stored (the
      // bootstrap value, before final_copy_w64 / reset_env_w64 take the row); an env that ended resets and
      // takes a second pass on its new initial obs, behind the reset's fence. The value of the row the
      // next action is taken from is the last pass's (an env that did not end: the bootstrap value).
      int passes = dn ? 2 : 1;  // wave-uniform
      asm volatile("" : "+s"(passes));
#pragma nounroll
      for (int ps = 0; ps < passes; ++ps) {
        if (ps) {
          final_copy_w64<MODE, OT>(R.F, A.B, N, (int)od, obs, nbr, TB.mask_out, env, rl);
          reset_env_w64<MODE, OT>(A.P, A.B, A.TP, TB, R.D, R.mt, (A.cur ^ (k + 1)) & 1, obs, nbr, env, rl, lds);
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __syncthreads();
        }
        // (the lane index opaque: else the row's addresses are computed before the step and held across it)
        int vl = (int)threadIdx.x;
        asm volatile("" : "+v"(vl));
        if (vl < N) {
          const size_t row = (size_t)env * N + vl;
          value_store_row(R.val, value_mlp_row<OT>(R.val, (int)od, obs + row * od), row, (size_t)k, kr, EN, A.traj != 0,
                          ps == 0);
        }
      }
    } else if (dn) {
      // behind the fence: the reset's stores follow the step's to the same rows (state, list, obs);
      // before them, the rows they overwrite go to the registered final outputs
      final_copy_w64<MODE, OT>(R.F, A.B, N, (int)od, obs, nbr, TB.mask_out, env, rl);
      reset_env_w64<MODE, OT>(A.P, A.B, A.TP, TB, R.D, R.mt, (A.cur ^ (k + 1)) & 1, obs, nbr, env, rl, lds);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __syncthreads();
    }
    if constexpr (!CARRY) {
      if (pol_in) {  // every agent row, as the bots kernel over all E x N rows; a reset env: its new initial obs
        uint8_t* const pol_out = A.traj ? pol_in + EN * abytes : pol_in;
        if (lane < N) {
          const size_t row = (size_t)env * N + lane;
          if constexpr (SMP)  // a reset env: the same decision index as the noise row k it would have read
            policy_sample_row<OT>(R.pol, R.smp, (int)od, obs, row, (size_t)k, kr, EN, pol_out);
          else if constexpr (POL)
            policy_act_row<OT>(R.pol, (int)od, obs, row, (size_t)k, kr, EN, pol_out);
          else if constexpr (TPOL)  // a reset env: init_health (the step's health output keeps the terminal one)
            tdm_policy_act_row<OT>(R.tpol, A.TP, TB, N, obs, lane, row, (size_t)k, kr, EN, dn != 0, pol_out);
          else if constexpr (MODE == kTdm)
            bot_combat_row(obs + row * (N - 1) * 4, TB.mask_out + row * (N - 1), N, pol_out + row * 4);
          else
            bot_flock_row(obs + row * od, (int)od, pol_out + row * 3);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __syncthreads();
      }
    }
  }
}

template <int MODE, int NCAP, typename OT, bool SCAL>
static void launch_roll_ar(const RolloutArgs<OT>& A, const FlockRollExtras& x, const ResetLaunch& r, int32_t* hit_out,
                           hipStream_t s) {
  const StepParams& P = A.P;
  if (A.B.sched && A.nsteps >= kRollBalanceMinSteps) {  // the balanced env order, as launch_roll
    if (launch_env_order(reinterpret_cast<const uint32_t*>(A.B.ccount[A.cur]), A.B.sched, P.n_envs, P.max_contacts, s) !=
        hipSuccess)
      return;  // no rollout on a stale order (the caller reports it)
  }
  RolloutArArgs<OT> R{};
  R.A = A;
  R.mt = r.mt;
  R.D = r.D;
  R.F = r.F;
  roll_variant<MODE, NCAP, OT>(R.A.cur, A.policy_act != nullptr, x, hit_out, [&](auto tag, auto carry, auto&& fill) {
    using OTA = typename decltype(tag)::type;
    RolloutArArgs<OTA> V;
    static_cast<RolloutArArgs<OT>&>(V) = R;
    fill(V);
    hipLaunchKernelGGL((env_rollout_ar_w64<MODE, NCAP, OTA, SCAL, decltype(carry)::value>), dim3(P.n_envs), dim3(W), 0, s,
                       V);
  });
}

hipError_t launch_rollout_ar_w64(const StepParams& P, const WorldBuffers& B, int cur, const FlockIO& io,
                                 const RollShape& sh, const FlockRollExtras& x, const ResetLaunch& r, hipStream_t s) {
  const TdmParams TP{};
  const TdmBuffers TB{};
  with_instance<kFlock>(P, io.obs_f64, [&](auto ncap, auto ot, auto scal) {
    using OT = decltype(ot);
    RolloutArgs<OT> A = roll_args<OT>(P, B, TP, TB, cur, io, sh, TailLaunch{});
    A.nbr_out = io.nbr;
    A.rew_out = io.rew;
    A.coll_out = io.coll;
    launch_roll_ar<kFlock, decltype(ncap)::value, OT, decltype(scal)::value>(A, x, r, nullptr, s);
  });
  return hipGetLastError();
}

hipError_t launch_tdm_rollout_ar_w64(const StepParams& P, const WorldBuffers& B, const TdmParams& TP,
                                     const TdmBuffers& TB, int cur, const TdmIO& io, const RollShape& sh,
                                     const ResetLaunch& r, hipStream_t s) {
  with_instance<kTdm>(P, io.obs_f64, [&](auto ncap, auto ot, auto scal) {
    using OT = decltype(ot);
    FlockRollExtras x;
    x.tdm_policy = io.policy;
    launch_roll_ar<kTdm, decltype(ncap)::value, OT, decltype(scal)::value>(
        roll_args<OT>(P, B, TP, TB, cur, io, sh, TailLaunch{}), x, r, io.hit_out, s);
  });
  return hipGetLastError();
}
