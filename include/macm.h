/*
 * macm.h — C-ABI of the MI355X-native batched gym-macm stepper (libmacm_hip.so).
 *
 * What this replaces (reference = siyarvurucu/gym-macm, file:line):
 *   - the per-env Box2D world owned by FrameworkBase
 *       gym_macm/cm_framework.py:155-167  (b2World(gravity=(0,0), doSleep=True))
 *       gym_macm/backends/no_render.py:4-19 (NoRender, the headless framework)
 *   - the body construction loop of Flock.__init__      gym_macm/envs/mvmnt.py:35-79
 *   - the whole env.step hot path                        gym_macm/envs/mvmnt.py:81-140
 *       action -> angle/force (:97-129), FrameworkBase.Step -> b2World.Step(1/60,8,3)
 *       + ClearForces (cm_framework.py:172-225), get_rewards (:160-179),
 *       time/done (:134-136), get_obs (:181-222)
 *
 * The reference's "API" at this boundary is pybox2d (SWIG) called per agent from
 * Python. Here one call advances E independent envs of N agents each, with all
 * per-agent arrays on the device (SoA), so control crosses host->device once per
 * step. No torch / C++ types cross this ABI: plain pointers, sizes, POD structs.
 *
 * Conventions
 *   - Every function returns int status: MACM_OK (0) or a negative MACM_E_* code;
 *     macm_last_error() returns a thread-local message for the last failure.
 *     Nothing aborts or throws across the ABI.
 *   - "device pointer" = memory the HIP runtime can dereference in a kernel
 *     (hipMalloc / torch CUDA tensor data_ptr()). Output buffers are borrowed for
 *     the duration of the call only; the world owns its state. (The one exception:
 *     macm_final_outputs, which a world keeps until they are replaced or cleared.)
 *   - stream = hipStream_t passed as void* (NULL = default stream). Calls are
 *     asynchronous on that stream; completion is the caller's synchronisation.
 *   - A world is bound to one device. Calls on one world are not thread-safe.
 */
#ifndef MACM_H
#define MACM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MACM_ABI_VERSION 9

enum {
  MACM_OK = 0,
  MACM_E_INVALID = -1,     /* bad argument / config / action (validate_actions) */
  MACM_E_OOM = -2,         /* device allocation failed                       */
  MACM_E_HIP = -3,         /* HIP runtime error                              */
  MACM_E_UNSUPPORTED = -4, /* config valid for the reference, not built here */
  MACM_E_OVERFLOW = -5     /* a per-env capacity overflowed in an earlier step: results since
                              then are not the reference's (reset / place / set_state clear it) */
};

enum { MACM_ACTION_DISCRETE = 0, MACM_ACTION_CONTINUOUS = 1 };
enum { MACM_REWARD_BINARY = 0, MACM_REWARD_LINEAR = 1 };
enum { MACM_COORD_POLAR = 0, MACM_COORD_CARTESIAN = 1 };

/*
 * Status bits accumulated per env on the device (macm_world_status). TOUCH/DEGREE are no longer
 * set (ABI 6): an env of either kind whose touching contacts exceed a fast kernel's LDS capacity
 * is stepped by the spill step (HBM working set sized by max_contacts) instead. CONTACT_OVERFLOW
 * (the fat-AABB pair list itself outgrew max_contacts; never for TDM, whose list holds every
 * pair) and SPILL_WAIT remain. Detection
 * is eventual, not synchronous: the kernels store the bits into a host-mapped word, and each step /
 * rollout call reads it before launching, without synchronising, so steps already queued behind an
 * overflowing one still run (and a rollout keeps stepping the overflowed env for its K steps); the
 * first call that sees the word returns MACM_E_OVERFLOW. macm_world_status() (which synchronises)
 * is exact. reset / place / set_state clear the bits; reset_envs re-derives the word from the envs
 * it did not reset.
 */
enum {
  MACM_ST_CONTACT_OVERFLOW = 1, /* Ov(F_t) list exceeded max_contacts                   */
  MACM_ST_TOUCH_OVERFLOW = 2,   /* (before ABI 6) TDM touching contacts beyond capacity  */
  MACM_ST_DEGREE_OVERFLOW = 4,  /* (before ABI 6) TDM body degree beyond capacity        */
  MACM_ST_INVALID_ACTION = 8,   /* validate_actions: an action outside the action space  */
  MACM_ST_SPILL_WAIT = 16,      /* a dense env found no free spill working-set slot for ~1 s
                                   (a pooled world: fewer slots than envs) and was not stepped */
  MACM_ST_HANDOFF = 32          /* workgroup path: kernel B's waves did not all start within ~1 s
                                   of B's dependencies finishing, or a kernel-C block waited ~1 s
                                   for B to hand it an env and skipped it (never expected: B's
                                   waves wait for nothing). Every env of the world carries the bit
                                   (the skipped env is unknown); results since then are invalid
                                   (ABI 8)                                                      */
};

/* macm_world_set_debug / macm_tdm_set_debug flags (test hooks; 0 = product behaviour; TDM takes
 * FORCE_SPILL, SPILL_POOL and SPILL_FAIL). */
enum {
  MACM_DEBUG_FORCE_SPILL = 1,     /* every env takes the spill step (parity tests of that path)  */
  MACM_DEBUG_SWEEP_CELLS = 2,     /* N > 64: pair sweep over strip cells at any N (else N >= 256) */
  MACM_DEBUG_SWEEP_ALL_PAIRS = 4, /* N > 64: all-pairs pair sweep at any N                        */
  MACM_DEBUG_SPILL_POOL = 8,      /* the spill working set as a pool of (flags >> 8) slots, at most
                                     the slots allocated (pooled-slot tests at small E)            */
  MACM_DEBUG_SPILL_FAIL = 16,     /* no spill slot is ever free: every env that needs the spill step
                                     is left unstepped with MACM_ST_SPILL_WAIT (ABI 8 test hook)   */
  MACM_DEBUG_ROLLOUT_RELOAD = 32, /* wave rollouts: every step loads its state from global memory
                                     behind a fence, none is carried in registers (A/B, tests)     */
  MACM_DEBUG_NEAR_PLAIN = 64      /* Flock wave rollouts: every step takes the all-pairs nearest-
                                     neighbour sweep, none the candidate lists (A/B, tests)        */
};

/*
 * macm_config — flockSettings (gym_macm/settings.py:110-146) + fwSettings
 * (settings.py:25-59) flattened. Field names follow the reference's attribute
 * names. macm_config_default() fills the reference defaults.
 */
typedef struct macm_config {
  int32_t n_agents;            /* sum(n_agents)                     mvmnt.py:61      */
  int32_t n_targets;           /* len(np.unique(targets))           mvmnt.py:42      */
  int32_t action_mode;         /* "discrete"/"continuous"           settings.py:136  */
  int32_t reward_mode;         /* "binary"/"linear"                 settings.py:137  */
  int32_t coord;               /* "polar"/"cartesian"               settings.py:141  */
  int32_t velocity_iterations; /* 8                                 settings.py:31   */
  int32_t position_iterations; /* 3                                 settings.py:32   */
  int32_t warm_starting;       /* enableWarmStarting = True         settings.py:34   */
  int32_t obs_f64;             /* 0: obs written as float32, 1: float64              */
  int32_t validate_actions;    /* 1: macm_world_step checks every action against the
                                  action space first (assert action_space.contains,
                                  mvmnt.py:94) and returns MACM_E_INVALID without
                                  stepping; synchronises the stream. 0 (default): no check */
  double hz;                   /* 60.0                              settings.py:30   */
  double start_spread;         /* 20                                settings.py:119  */
  double start_point[2];       /* [0, 0]                            settings.py:120  */
  double agent_rotation_speed; /* 0.8 * 2pi                         settings.py:121  */
  double agent_force;          /* 20                                settings.py:122  */
  double time_limit;           /* 60                                settings.py:123  */
  double reward_radius;        /* 7 if binary else 1                settings.py:146  */
  double target_mindist;       /* 25                                settings.py:139  */
  double target_maxdist;       /* 60                                settings.py:140  */
  float radius;                /* circle r = 0.5                    settings.py:127-131 */
  float density;               /* 1                                                  */
  float friction;              /* 0.3                                                */
  float linear_damping;        /* 5                                 settings.py:133  */
} macm_config;

/*
 * macm_tdm_config — the team-deathmatch env (gym_macm/envs/combat.py:13-264,
 * combatSettings settings.py:149-177). The reference's TDM cannot be built as
 * shipped (combat.py:65 NameError; :150-151,173 read attributes that do not
 * exist); this is its semantics with those four names supplied from
 * combatSettings, everything else literal (see DESIGN.md "TDM").
 */
typedef struct macm_tdm_config {
  int32_t n_teams;              /* len(n_agents)                      combat.py:70-73 */
  int32_t team_size[4];         /* n_agents[i]                                        */
  int32_t n_agents;             /* sum(n_agents) (<= 4096; > 64: the workgroup step)   */
  int32_t velocity_iterations;  /* 8                                                  */
  int32_t position_iterations;  /* 3                                                  */
  int32_t warm_starting;        /* 1                                                  */
  int32_t obs_f64;              /* obs written as float32 (0) or float64 (1)          */
  int32_t fresh_raycast;        /* 0 (reference): ONE RayCastClosestCallback whose hit /
                                   fixture are never reset (cm_framework.py:62-65,76,
                                   combat.py:147-153), so after the first hit every
                                   attack damages the last-hit body. 1: per-cast hit.  */
  int32_t decay_mov_penalty;    /* 0 (reference): cooldown_mov_penalty is never
                                   decremented (combat.py:151,155). 1: decremented by
                                   1/hz alongside cooldown_atk.                        */
  int32_t validate_actions;     /* 1: macm_tdm_step checks the alive agents' actions
                                   (assert action_space.contains, combat.py:118) first,
                                   MACM_E_INVALID without stepping; synchronises          */
  int32_t _pad;
  double hz;                    /* 60                                                 */
  double world_width;           /* 30                                 combat.py:76    */
  double world_height;          /* 30                                 combat.py:77    */
  double agent_rotation_speed;  /* 0.8 * 2pi                          combat.py:18    */
  double agent_force;           /* 20                                 combat.py:19    */
  double percent_mov_penalty;   /* 0.2                                combat.py:22    */
  double melee_range;           /* 2                                  combat.py:20    */
  double melee_dmg;             /* 0.25                               combat.py:21    */
  double init_health;           /* 1                                  combat.py:14    */
  double cooldown_atk;          /* 1                                  settings.py:164 */
  double cooldown_mov_penalty;  /* 0.5                                settings.py:165 */
  double time_limit;            /* 60                                 settings.py:163 */
  float radius, density, friction, linear_damping;
} macm_tdm_config;

/*
 * Device-side outputs of one TDM step (device pointers; NULL = not wanted).
 * TDM.get_obs (combat.py:206-227) as fixed slots: slot k of agent i is agent
 * j = k < i ? k : k + 1 and holds (r, t, p, is_ally); the dict API lists the alive
 * j in the same order. mask = agents i and j both alive; masked slots are zero.
 */
typedef struct macm_tdm_outputs {
  void* obs;        /* [E, N, N-1, 4] float32 or float64 (config.obs_f64)     */
  uint8_t* mask;    /* [E, N, N-1]                                           */
  double* health;   /* [E, N]  Agent.health                                  */
  uint8_t* alive;   /* [E, N]  Agent.alive                                   */
  uint8_t* done;    /* [E]     TDM.done (latches)                            */
  int32_t* winner;  /* [E]     TDM.winner, -1 = None                         */
} macm_tdm_outputs;

/*
 * TDM state, SoA (host or device pointers, NULL = skip). Physics fields as
 * macm_state; plus
 *   health, cd_atk, cd_mov [E, N] float64   Agent.health / cooldown_atk / cooldown_mov_penalty
 *   alive                  [E, N] uint8
 *   listener               [E, 2] int32     (RayCastClosestCallback.hit, body of .fixture or -1)
 *   done [E] uint8, winner [E] int32
 *   contact_stride         entries per env row of the caller's contact_ab / contact_imp, as
 *                          macm_state (0 = C = N(N-1)/2; ABI 7: a stride of max(contact_count)
 *                          moves only the lists' used part, C is 523,776 at N = 1024)
 */
typedef struct macm_tdm_state {
  void* pos;
  void* vel;
  void* angle;
  void* fat;
  void* sleep;
  void* health;
  void* cd_atk;
  void* cd_mov;
  void* alive;
  void* listener;
  void* contact_count;
  void* contact_ab;
  void* contact_imp;
  void* step_count;
  void* time_passed;
  void* done;
  void* winner;
  int64_t contact_stride;
} macm_tdm_state;

/*
 * Device-side outputs of one step (all device pointers; NULL = not wanted,
 * except reward which is required). Shapes: E = n_envs, N = n_agents,
 * OD = 4 (polar: nbr r, nbr t, target r, target t) or 6 (cartesian: nbr r,
 * cos t, sin t, target r, cos t, sin t). Matches Flock.get_obs node order
 * (mvmnt.py:197-220): node 0 = closest agent (type 0, id = nbr_id), node 1 =
 * the agent's target (type 1, id = N).
 *
 * Alignment (macm_tdm_outputs too): obs must be 16-byte aligned, the kernels store a polar float32 row
 * and every TDM slot as one 16-byte vector (float64: two); every other field needs its element type's
 * alignment only (a TDM mask that is 16-byte aligned lets the tail observation store it in 16-byte
 * pieces, any other is stored by bytes). A kernel writes only inside the [E, ...] (trajectory form:
 * [n_steps, E, ...]) extent of the fields that are set.
 */
typedef struct macm_outputs {
  void* obs;        /* [E, N, OD] float32 or float64 (config.obs_f64)          */
  int32_t* nbr_id;  /* [E, N] index of the closest other agent                 */
  float* reward;    /* [E, N] -1 in any contact, else binary 0/1 or linear     */
  uint8_t* collided;/* [E, N] 1 if the agent is in world.contacts              */
  uint8_t* done;    /* [E] time_passed > time_limit                            */
} macm_outputs;

/*
 * World state, SoA. Used by get/set_state (parity injection, checkpoints).
 * Pointers may be host or device memory (copied with hipMemcpyDefault).
 *   pos, vel      [E, N, 2] float32   body position (sweep c) / linear velocity
 *   angle         [E, N]    float32   sweep angle
 *   fat           [E, N, 4] float32   broad-phase fat AABB (lo.x, lo.y, hi.x, hi.y)
 *   sleep         [E, N]    float32   sleepTime
 *   targets       [E, T, 2] float32
 *   contact_count [E]       int32     length of the ordered contact list
 *   contact_ab    [E, C]    uint32    a | b << 16, a < b, Box2D world-list order
 *   contact_imp   [E, C, 2] float32   (normalImpulse, tangentImpulse) warm start
 *   step_count    [E]       int32     steps taken (0 => dtRatio 0 on next step)
 *   time_passed   [E]       float64
 *   contact_stride            entries per env row of the caller's contact_ab / contact_imp
 *                             (0 = C = macm_world_info().max_contacts). get_state fills the first
 *                             min(stride, C) entries of each row: a stride of max(contact_count)
 *                             moves only the lists' used part (ABI 5; C can be large for N > 64).
 */
typedef struct macm_state {
  void* pos;
  void* vel;
  void* angle;
  void* fat;
  void* sleep;
  void* targets;
  void* contact_count;
  void* contact_ab;
  void* contact_imp;
  void* step_count;
  void* time_passed;
  int64_t contact_stride;
} macm_state;

typedef struct macm_world_info {
  int32_t n_envs, n_agents, n_targets, obs_dim;
  int32_t max_contacts;   /* per-env ordered contact list capacity */
  int32_t max_touching;   /* per-env solver capacity               */
  int32_t device;
  int32_t spill_slots;    /* spill working-set slots (= n_envs: one per env; fewer: a pool) */
  int32_t launch_flags;   /* MACM_LAUNCH_* of the workgroup step, decided at the first step (ABI 8) */
  int32_t rollout_slices; /* env slices a workgroup-path rollout runs on streams of their own (0: none;
                             MACM_WG_SLICES overrides the default 3) (ABI 9)                       */
} macm_world_info;

/* macm_world_info.launch_flags */
#define MACM_LAUNCH_HANDOFF 1  /* kernel C as kernel B's consumer on a second stream (MACM_HANDOFF) */
#define MACM_LAUNCH_SPLIT_OBS 2 /* TDM (macm_tdm_launch_flags, ABI 9): the step writes pose snapshots and
                                   tdm_observe_snap observes them in a launch of its own (fewer than
                                   1024 envs, N <= 64; MACM_TDM_SPLIT_OBS overrides); same results */
#define MACM_LAUNCH_TAIL_OBS 4  /* TDM trajectory rollouts (macm_tdm_rollout_traj): the tail observation,
                                   each env's wave steps its K steps writing pose snapshots, then the
                                   finished waves and observe-only waves observe the (step, env) rows
                                   (fewer than 2048 envs, N <= 64, the launch resident at once;
                                   MACM_TDM_TAIL_OBS overrides); same results */

typedef struct macm_world macm_world;

/* Library identity. */
const char* macm_version(void);
int macm_abi_version(void);
const char* macm_last_error(void);

/* Reference defaults (settings.py:25-59, 110-146). */
int macm_config_default(macm_config* cfg);

/*
 * Create E envs of one Flock configuration on `device`.
 *   targets_idx: host int32[N], agent -> target index (mvmnt.py:43), or NULL = all 0.
 *   max_contacts: per-env capacity C of the ordered fat-AABB pair list (and of each slot of
 *   the spill step's HBM working set). 0 = the default, from a budget of 1/8 of the device's
 *   free memory at creation (so every world shrinks what the next one sees), half for the lists
 *   (24 B per entry and env): N(N-1)/2 (every pair: the list can never overflow) when N <= 64 or
 *   when that fits, otherwise the largest C that fits (at least 32 N). The other half holds the
 *   spill working set, 48 B per entry and 48 B per body per slot: one slot per env when they fit,
 *   otherwise a pool (>= 16 slots) that dense envs take turns on (macm_world_info: spill_slots).
 *   On an idle 288 GB MI355X: C5's shard (2048 envs x 1024 agents) gets C ~ 366k and ~1k slots.
 *   Overflow of the list sets MACM_ST_CONTACT_OVERFLOW and a later step returns MACM_E_OVERFLOW.
 * Replaces: Flock.__init__ world + body creation (mvmnt.py:35-79,
 * cm_framework.py:155-167). State is undefined until macm_world_reset.
 */
int macm_world_create(const macm_config* cfg, const int32_t* targets_idx, int32_t n_envs,
                      int32_t device, int32_t max_contacts, macm_world** out);
int macm_world_destroy(macm_world* w);
int macm_world_info_get(const macm_world* w, macm_world_info* info);

/*
 * Initialise every env exactly as Flock.__init__ would after
 * random.seed(seed + env_offset + e) (CPython MT19937; mvmnt.py:47-79 draw order:
 * targets (angle, dist) then agents (x, y, angle)). Resets time, contacts, status.
 * Writes the initial observation (Flock.obs, mvmnt.py:79) into `out` if non-NULL.
 * Every env's seed is taken modulo 2^64 as a key of one or two 32-bit words, which is random.seed's
 * meaning only for seed + env_offset + e in [0, 2^64): CPython seeds a negative int by its absolute
 * value and an int of 2^64 or more by a longer key. The caller keeps seed >= 0 and the envs' seeds in
 * that range (macm_tdm_reset too); the Python handles raise ValueError outside it.
 */
int macm_world_reset(macm_world* w, uint64_t seed, int64_t env_offset, const macm_outputs* out,
                     void* stream);

/*
 * Like macm_world_reset, but with caller-drawn poses (host or device pointers):
 * pos [E, N, 2] float32, angle [E, N] float32, targets [E, T, 2] float32. Used by
 * the drop-in Flock facade, which draws them from Python's global `random` in
 * the reference's order (mvmnt.py:47-64) so the caller's RNG stream advances
 * exactly as the reference's would.
 */
int macm_world_place(macm_world* w, const void* pos, const void* angle, const void* targets,
                     const macm_outputs* out, void* stream);

/*
 * Start a new episode in the envs selected by env_mask (device or host uint8 [E],
 * nonzero = reset; NULL = all), e.g. the done flags of the last step. Each env
 * continues the CPython MT19937 stream macm_world_reset seeded it with, drawing
 * the next agent poses exactly as the reference's reset() draws them from the
 * global `random` (mvmnt.py:224-233, targets kept); velocities, sleep clocks,
 * contacts, time and done restart. The new episodes' initial obs are written into
 * `out` for the reset envs only. Asynchronous on `stream` (no host round trip).
 * Fails with MACM_E_INVALID after macm_world_place (no device streams).
 */
int macm_world_reset_envs(macm_world* w, const uint8_t* env_mask, const macm_outputs* out, void* stream);

/*
 * Autoreset (off at creation; on != 0 turns it on). With it on, an env whose step sets `done` starts
 * its next episode before its next step, exactly as macm_world_reset_envs would with that step's
 * done flags as the mask (the env's stream continued, targets kept), in macm_world_step and inside
 * every rollout: on the wave path (N <= 64) the env's own wave resets it within the launch, on the
 * workgroup path the draw and init launches follow each step's on the same stream (such rollouts
 * run without env slices: macm_world_info.rollout_slices is 0). The usual vector-env convention
 * holds for the outputs of such a step (row k of a trajectory): done (1), reward and collided are
 * the terminal values as the step wrote them; obs and nbr_id of the reset envs are the new
 * episode's initial observation (NULL fields stay unwritten), and the closed loop's next action of
 * a reset env is taken from it. Counters, reward sums and spilled are those of the loop
 * step -> reset_envs(done) [-> bots]. A reset env's device status word is rewritten as by
 * reset_envs; the host-mapped status word (what makes a step return MACM_E_OVERFLOW) stays set
 * until the next macm_world_reset / reset_envs / place / set_state: a reset inside a launch cannot
 * resync it. With autoreset on and no device streams (the world was placed, not reset) step and
 * every rollout return MACM_E_INVALID with reset_envs' message and launch nothing. A NULL world gives
 * MACM_E_INVALID. Additive: no struct changed, MACM_ABI_VERSION stays 9.
 * The obs and nbr_id that the reset overwrites are kept where macm_world_set_final_outputs says.
 */
int macm_world_set_autoreset(macm_world* w, int32_t on);

/*
 * Where an autoreset world keeps what the reset would otherwise overwrite (device pointers,
 * NULL = not wanted): the observation an episode ended on, which value bootstrapping at a time-limit
 * truncation needs (gym's info["terminal_observation"] / final_observation).
 *
 * Lifetime: the world keeps a copy of this struct, not of the buffers, until
 * macm_*_set_final_outputs replaces or clears it (fin NULL, or every field NULL) or the world is
 * destroyed; the caller keeps the buffers alive that long. This is the one exception to "outputs are
 * borrowed for the call".
 *
 * With autoreset on, whenever the step of env e sets done, row e of every set field is written before
 * the reset touches the step's output row, in macm_*_step and in every rollout form, on every path:
 *   obs, nbr_id (TDM: obs, mask)  what that step wrote to its output row (row k of a trajectory), bit
 *                                 for bit what the same step returns with autoreset off;
 *   length[e]                     the ended episode's env steps;
 *   ends[e]                       incremented by 1.
 * Rows of envs that did not end are not touched; with autoreset off nothing is ever written; reset,
 * reset_envs and place never write. The slots are per env, not per trajectory row: if an env ends more
 * than once inside one launch, the last end's values remain and ends counts all of them (a caller that
 * needs every end keeps n_steps at or below the shortest possible episode, or reads ends).
 * The rows are copied from the call's output row, so a call on an autoreset world with fin.obs set
 * needs its own out / traj obs set, and likewise nbr_id and mask: otherwise it returns MACM_E_INVALID
 * and steps no env.
 */
typedef struct macm_final_outputs {
  void*    obs;     /* Flock [E, N, OD], TDM [E, N, N-1, 4]; float32/float64 as config.obs_f64; 16-byte aligned */
  int32_t* nbr_id;  /* Flock [E, N]; ignored by TDM   */
  uint8_t* mask;    /* TDM [E, N, N-1]; ignored by Flock */
  int32_t* length;  /* [E] env steps of the episode that ended (step_count after its last step) */
  int32_t* ends;    /* [E] += 1 at every episode end of env e (the caller zeroes it) */
} macm_final_outputs;

/* NULL or all-NULL: none. MACM_E_INVALID for a NULL world or an obs that is not 16-byte aligned
 * (nothing changes then). Additive: MACM_ABI_VERSION stays 9. */
int macm_world_set_final_outputs(macm_world* w, const macm_final_outputs* fin);

/*
 * One env.step for all E envs.
 *   actions: device pointer. Discrete: uint8/int8 [E, N, 3] in {0,1,2}
 *   (MultiDiscrete([3,3,3]), mvmnt.py:143-145). Continuous: float32 [E, N, 2] in [-1,1].
 * Replaces Flock.step (mvmnt.py:81-140) incl. b2World.Step(1/hz, 8, 3) + ClearForces.
 * Returns MACM_E_OVERFLOW (and launches nothing) if an earlier step or reset set a status bit
 * (read from a host-mapped word the kernels write; no synchronisation). With
 * cfg.validate_actions, returns MACM_E_INVALID and steps no env if any action is outside the
 * action space (reference: AssertionError before any agent acts, mvmnt.py:94).
 */
int macm_world_step(macm_world* w, const void* actions, const macm_outputs* out, void* stream);

/*
 * n_steps consecutive env.steps of all E envs with actions given in advance, e.g. the
 * reference's random-action loop (`env.step(env.action_space.sample())`, mvmnt.py:271-293),
 * in one launch on the wave path (N <= 64): each env's wave runs its steps back to back, so no
 * env waits at a launch boundary for the slowest env of the batch. Results are those of
 * n_steps macm_world_step calls with the same actions.
 *   actions: device pointer, [n_steps, E, N, 3] uint8 (discrete) or [n_steps, E, N, 2] float32.
 *   out: overwritten by every step; the last step's outputs remain. Counters accumulate all steps.
 * The workgroup path (N > 64) launches its steps one after another. n_steps = 0 does nothing
 * (actions may then be NULL).
 * With cfg.validate_actions every step's actions are checked before any env is stepped.
 */
int macm_world_rollout(macm_world* w, const void* actions, int32_t n_steps, const macm_outputs* out, void* stream);

/*
 * n_steps of the closed loop `step -> bots.flock -> step` (test_scripts/bots.py:37-61 acting on every
 * agent's observation, as macm_bots_flock) in one launch on the wave path: each env's wave steps,
 * then every lane takes its agent's next action from the observation just written.
 *   actions: device uint8 [E, N, 3]; in: the first step's actions (e.g. macm_bots_flock on the
 *   initial obs); out: the bot's actions for the step after the last. out->obs must be set.
 * Same results as n_steps of (macm_world_step, macm_bots_flock). Workgroup path: those launches.
 */
int macm_world_rollout_bots(macm_world* w, uint8_t* actions, int32_t n_steps, const macm_outputs* out, void* stream);

/*
 * Trajectory forms: as macm_world_rollout / macm_world_rollout_bots, but every step's outputs are
 * kept, as the reference returns (obs, rewards) from every env.step (mvmnt.py:140): each non-NULL
 * field of `traj` is a [n_steps, ...] buffer whose row k receives step k's outputs
 * (obs [n_steps, E, N, OD], nbr_id / reward / collided [n_steps, E, N], done [n_steps, E]).
 * Bots form: actions is [n_steps + 1, E, N, 3]; row 0 holds the first step's actions on entry and
 * step k writes the bot's actions for step k + 1 into row k + 1, so (obs, action, reward) of every
 * step stay in HBM. Same results as the per-step calls; one launch on the wave path (ABI 5).
 */
int macm_world_rollout_traj(macm_world* w, const void* actions, int32_t n_steps, const macm_outputs* traj,
                            void* stream);
int macm_world_rollout_bots_traj(macm_world* w, uint8_t* actions, int32_t n_steps, const macm_outputs* traj,
                                 void* stream);

/*
 * A learned policy as the actor of the closed loop: a float32 MLP over every agent's obs row, in the
 * place of the scripted bot, so that a collector gets n_steps of (obs, action, logits, reward, done,
 * final obs) from one launch. Defined so that it can be checked bit for bit; all arithmetic float32:
 *   input   x[q] = (float)obs[q], q < in_dim, the row as stored (float64 obs round to nearest);
 *   layer   acc = b[j], then acc = fmaf(W[k][j], x[k], acc) for k = 0, 1, ... ascending: one rounding
 *           per step, no other association;
 *   hidden  relu(v) = v > 0 ? v : +0.0f (-0 and NaN give +0); the output layer has no activation;
 *   output  9 logits, head h in {0, 1, 2} of MultiDiscrete([3, 3, 3]) at logits[3h + c];
 *   action  z[c] = logits[3h + c] + noise[3h + c] (one float32 add; without noise z[c] = logits[3h + c]);
 *           action[h] = the lowest c with the largest z: best = 0, top = -inf, then for c = 0, 1, 2
 *           `if (z[c] > top) best = c, top = z[c]`, so a NaN is never chosen over a number.
 * Denormals are kept; the sign and payload of a NaN logit are unspecified. The caller supplies the noise (Gumbel noise for sampling; NULL: the argmax) as
 * it supplies the actions of macm_world_rollout, or has the launch draw it (macm_sample_config, below:
 * only where the noise comes from changes, the action rule above stays word for word);
 * the learner recomputes log-probabilities from the stored logits.
 *   params: device float32, 16-byte aligned, row-major [in][out]:
 *           W1[in_dim][hidden], b1[hidden], (W2[hidden][hidden], b2[hidden] if n_hidden == 2),
 *           W3[hidden][9], b3[9].
 * hidden is 16 or 32, n_hidden 1 or 2, in_dim 4 (polar) or 6 (cartesian), reserved 0.
 * Flock worlds with discrete actions only: a TDM observation is a masked set, not a fixed vector, and
 * has a policy of its own (macm_tdm_policy, below); continuous actions have no heads (out of scope).
 * Additive: MACM_ABI_VERSION stays 9.
 */
typedef struct macm_policy_mlp {
  int32_t in_dim, hidden, n_hidden, reserved;
  const float* params;
} macm_policy_mlp;

/*
 * The policy's decision for `rows` obs rows ([rows, in_dim], float32 or float64 as obs_f64), as
 * macm_bots_flock is for the bot: the first actions of a closed loop from the initial obs, and what
 * the per-step loop calls. noise [rows, 9] or NULL; actions uint8 [rows, 3]; logits [rows, 9] or NULL.
 * MACM_E_INVALID: p NULL or outside the shapes above, params NULL or misaligned, obs or actions NULL.
 */
int macm_policy_flock(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows, const float* noise,
                      uint8_t* actions, float* logits, void* stream);

/*
 * Registers the policy of macm_world_rollout_policy. A registration, as macm_world_set_final_outputs:
 * the world keeps a copy of the struct, not of the params buffer, until it is replaced, cleared (p
 * NULL) or the world is destroyed; the learner may overwrite params between launches, and the next
 * launch reads the new values. MACM_E_INVALID, nothing changed: a NULL world, a struct outside the
 * shapes above, params NULL or misaligned, in_dim other than the world's obs_dim.
 * MACM_E_UNSUPPORTED: a continuous-action world.
 */
int macm_world_set_policy(macm_world* w, const macm_policy_mlp* p);

/*
 * n_steps of the closed loop `step -> policy -> step`, as macm_world_rollout_bots / _bots_traj with
 * the registered policy as the actor: one launch on the wave path (N <= 64); on the other paths the
 * launches of macm_world_step and macm_policy_flock on the caller's stream (no env slices).
 *   actions: [E, N, 3] in and out; trajectory form [n_steps + 1, E, N, 3], row 0 given, step k writes row k + 1.
 *   noise:   [n_steps, E, N, 9] or NULL; row k is used for the decision taken after step k.
 *   logits:  [E, N, 9] (the last step's remain), trajectory form [n_steps, E, N, 9], or NULL; row k
 *            holds the logits computed from obs row k.
 * With autoreset on, a reset env's next action comes from its new initial obs (which is what obs row
 * k then holds), as for the bots; the final outputs are written as in every other form.
 * out->obs must be set. MACM_E_INVALID without a registered policy. n_steps = 0 does nothing.
 * Same results as n_steps of (macm_world_step, macm_policy_flock).
 */
int macm_world_rollout_policy(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                              const macm_outputs* out, void* stream);
int macm_world_rollout_policy_traj(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise,
                                   float* logits, const macm_outputs* traj, void* stream);

/*
 * In-launch action sampling: the policy draws its own Gumbel noise from a counter-based generator, so
 * that sampling from softmax(logits) needs no [n_steps, E, N, 9] noise tensor, and the noise of a
 * decision is reproducible from (seed, decision index, env, agent, head) however the steps are cut
 * into launches. For decision index d (uint64), flat row r = e * n_agents + i of the call or world,
 * the job's row first_row of that row 0 (below; 0 unless named) and head h:
 *   words   w[0..3] = Philox4x32-10(counter = (first_row + r, lo32(d), hi32(d), h), key = (lo32(seed), hi32(seed))),
 *           the standard generator (multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9
 *           and 0xBB67AE85, 10 rounds); word c < 3 belongs to logit 3h + c, word 3 is unused;
 *   uniform u = ((double)w + 0.5) * 2^-32: exact in float64 and strictly inside (0, 1);
 *   noise   g = (float)(-log(-log(u))): both logarithms the device library's float64 log, every
 *           operation rounded once, one final rounding to float32;
 *   action  z[c] = logits[3h + c] + g, the float32 add and the rule of macm_policy_mlp.
 * In a rollout the decision taken after step k of a launch (the one noise row k serves) has
 * d = decision + k, `decision` being the world's counter at the call; a reset env's decision on its
 * new initial obs has the same d. reserved is 0. Additive: MACM_ABI_VERSION stays 9.
 *
 * first_row: the counter's row word is first_row + r, so that a call over some rows of a job, or a world
 * that holds a shard of its envs, draws what the whole job draws for those rows: the rank whose envs are
 * [e0, e0 + E) of the job names first_row = e0 * n_agents, and its agent (e, i) then draws as the job's
 * (e0 + e, i). first_row is in [0, 2^32] and first_row + rows <= 2^32 (for a world rows = E * n_agents):
 * the word never wraps. The entry points with _at take it; those without are the _at ones with
 * first_row = 0, in every bit. With one seed and first_row = 0 on every rank, local agent (e, i) of every
 * rank draws the same noise at every decision.
 */
typedef struct macm_sample_config {
  uint64_t seed, decision;
  int32_t reserved[4];
} macm_sample_config;

/*
 * The noise that decisions cfg->decision .. cfg->decision + n_dec - 1 draw for rows r < rows, float32
 * [n_dec, rows, 9]: what a launch with sampling on adds to its logits, bit for bit, so that a launch
 * given this buffer as `noise` is its twin. words: the generator's raw output, uint32 [n_dec, rows, 3, 4]
 * (head h, word q at [.., h, q]), or NULL.
 * MACM_E_INVALID, nothing launched: cfg NULL, reserved != 0, n_dec < 0, rows < 0 or rows > 2^32 (r is a
 * 32-bit word), noise NULL. n_dec = 0 or rows = 0 writes nothing.
 */
int macm_policy_noise(const macm_sample_config* cfg, int64_t n_dec, int64_t rows, float* noise, uint32_t* words,
                      void* stream);
/*
 * ... for the job's rows first_row <= r' < first_row + rows: element [j, r] is the noise of the job's row
 * first_row + r, so the buffer is rows [first_row, first_row + rows) of the job's macm_policy_noise.
 * MACM_E_INVALID, nothing launched: as macm_policy_noise, and first_row < 0 or first_row + rows > 2^32.
 */
int macm_policy_noise_at(const macm_sample_config* cfg, int64_t first_row, int64_t n_dec, int64_t rows, float* noise,
                         uint32_t* words, void* stream);

/*
 * macm_policy_flock with the draw inside: row r decides at decision cfg->decision, with the bits of
 * macm_policy_flock given macm_policy_noise(cfg, 1, rows). The first actions of a sampled closed loop
 * (decision 0, the world's sampling then starting at decision 1), and what the per-step loop calls.
 * MACM_E_INVALID, nothing launched: as macm_policy_flock, and cfg NULL, reserved != 0, rows > 2^32.
 */
int macm_policy_flock_sampled(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows,
                              const macm_sample_config* cfg, uint8_t* actions, float* logits, void* stream);
/*
 * ... with row r of obs drawing as the job's row first_row + r: the first actions of a shard's closed loop,
 * with the bits of macm_policy_flock given macm_policy_noise_at(cfg, first_row, 1, rows).
 * MACM_E_INVALID, nothing launched: as macm_policy_flock_sampled, and first_row < 0 or
 * first_row + rows > 2^32.
 */
int macm_policy_flock_sampled_at(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t first_row,
                                 int64_t rows, const macm_sample_config* cfg, uint8_t* actions, float* logits,
                                 void* stream);

/*
 * Sampling as a property of the world, like autoreset; off at creation. While it is on,
 * macm_world_rollout_policy / _traj / _value / _value_traj called with noise == NULL draw: the decision
 * after step k uses d = decision + k, and a call that launched advances the world's host-side
 * `decision` by n_steps (no synchronisation). One launch on the wave path, whose kernels are
 * instantiations of their own; on the other paths the per-step loop calls the sampled one-shot kernel
 * with d = decision + k, which gives the same draws. A call with noise given while sampling is on
 * returns MACM_E_INVALID, and nothing is launched. cfg NULL turns sampling off: everything is as
 * before, and noise == NULL is the argmax again.
 * MACM_E_INVALID, nothing changed: a NULL world, reserved != 0. MACM_E_UNSUPPORTED: a continuous-action
 * world.
 * macm_world_get_sampling: 1 with sampling on, *cfg_out the seed and the decision the next launch
 * starts at; 0 with sampling off, *cfg_out zeroed; MACM_E_INVALID for a NULL argument.
 * macm_world_set_sampling_at: the world's row 0 draws as the job's row first_row (a world created with
 * env_offset e0 as a shard of a job: e0 * n_agents), on every path and in every policy rollout, so that
 * the shard's sampled launches have the bits of the whole job's for its envs. Also MACM_E_INVALID, nothing
 * changed (an earlier registration stays): first_row < 0, first_row + E * n_agents > 2^32. cfg NULL
 * clears first_row to 0 with the rest. macm_world_set_sampling is this with first_row = 0.
 * macm_world_get_sampling_row: *first_row as registered (0 with sampling off), the return value that of
 * macm_world_get_sampling; MACM_E_INVALID for a NULL argument.
 */
int macm_world_set_sampling(macm_world* w, const macm_sample_config* cfg);
int macm_world_get_sampling(macm_world* w, macm_sample_config* cfg_out);
int macm_world_set_sampling_at(macm_world* w, const macm_sample_config* cfg, int64_t first_row);
int macm_world_get_sampling_row(macm_world* w, int64_t* first_row);

/*
 * A critic beside the actor: a second float32 MLP over the same obs row, with a trunk of its own and
 * one output, V(obs), so that a PPO / A2C collector gets the values of every row and the bootstrap
 * value of every step from the launch that steps the envs. The arithmetic is macm_policy_mlp's, word
 * for word: x[q] = (float)obs[q]; each layer the k-ordered fmaf chain from the bias, one rounding per
 * step; relu(v) = v > 0 ? v : +0.0f on the hidden layers, none on the last. Denormals are kept; the
 * sign and payload of a NaN are unspecified.
 *   params: device float32, 16-byte aligned, row-major [in][out]:
 *           W1[in_dim][hidden], b1[hidden], (W2[hidden][hidden], b2[hidden] if n_hidden == 2),
 *           W3[hidden][1], b3[1].
 * hidden is 16 or 32, n_hidden 1 or 2, in_dim 4 (polar) or 6 (cartesian), reserved 0; the critic's
 * shape is independent of the actor's. Additive: MACM_ABI_VERSION stays 9.
 */
typedef struct macm_value_mlp {
  int32_t in_dim, hidden, n_hidden, reserved;
  const float* params;
} macm_value_mlp;

/*
 * V of `rows` obs rows ([rows, in_dim], float32 or float64 as obs_f64) into values [rows]: the values
 * of a rollout's first row, and what the per-step loop calls.
 * MACM_E_INVALID: c NULL or outside the shapes above, params NULL or misaligned, obs or values NULL,
 * rows < 0. rows = 0 writes nothing.
 */
int macm_value_flock(const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t rows, float* values,
                     void* stream);

/*
 * Registers the critic of macm_world_rollout_policy_value: a registration, as macm_world_set_policy
 * (the world keeps the struct, not the params buffer; the learner may overwrite params between
 * launches; c NULL clears). MACM_E_INVALID, nothing changed: a NULL world, a struct outside the shapes
 * above, reserved != 0, params NULL or misaligned, in_dim other than the world's obs_dim.
 * MACM_E_UNSUPPORTED: a continuous-action world. A world with a critic registered runs every other
 * entry point exactly as without one.
 */
int macm_world_set_critic(macm_world* w, const macm_value_mlp* c);

/*
 * macm_world_rollout_policy / _traj, bit for bit, and in addition for step k of env e:
 *   boot   row k receives V of the observation step k produced, before any reset. With autoreset on,
 *          in a step that sets done, that is the row that goes to the final outputs' obs: every end
 *          inside the launch has its bootstrap value, where the final outputs keep only an env's last
 *          end. (4 B per agent-step; the terminal observation row itself is not kept per trajectory
 *          row: it would double the largest buffer, and its main use is this number.)
 *   values row k + 1 receives V of the observation the action of step k + 1 is taken from: obs row k as
 *          it stands after the step and any reset (a reset env: its new initial obs). When the env
 *          did not end, values[k + 1] and boot[k] hold the same bits.
 * Trajectory form: values [n_steps + 1, E, N], row 0 is the caller's (macm_value_flock on the
 * initial obs) and is neither read nor written; boot [n_steps, E, N]. Overwrite form: values [E, N],
 * V of the obs the returned next actions come from; boot [E, N], the last step's bootstrap value.
 * Either of values and boot may be NULL: not wanted, never stored to. Both NULL: MACM_E_INVALID (the
 * plain entry point serves that case). MACM_E_INVALID, nothing changed or launched, without a
 * registered critic or policy. n_steps = 0 does nothing. One launch on the wave path (N <= 64); on
 * the other paths the launches of the per-step loop. Same results as n_steps of
 *   macm_world_step, macm_value_flock (boot), [reset_envs(done)], macm_policy_flock, macm_value_flock (values).
 */
int macm_world_rollout_policy_value(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise,
                                    float* logits, float* values, float* boot, const macm_outputs* out,
                                    void* stream);
int macm_world_rollout_policy_value_traj(macm_world* w, uint8_t* actions, int32_t n_steps, const float* noise,
                                         float* logits, float* values, float* boot, const macm_outputs* traj,
                                         void* stream);

/*
 * Generalised advantage estimation over a trajectory, any env kind, all float32. reward, values, boot,
 * adv and ret are [n_steps, E, N] (values may point at the first n_steps rows of the launch's
 * [n_steps + 1, E, N] buffer); done is [n_steps, E], any nonzero byte counts as done. values[k] is V of
 * the observation the action of step k was taken from, so adv[k] and ret[k] belong to action row k of
 * macm_world_rollout_policy_value_traj, the decision taken from obs row k - 1 (logits row k - 1), and
 * values[:n_steps] to the decisions of action rows 0 .. n_steps - 1: not to obs row k, which step k
 * wrote. A learner pairs obs[j], logits[j], actions[j + 1] and values[j + 1] with reward[j + 1],
 * done[j + 1] and boot[j + 1] (all leading-dimension slices of the buffers) and runs this on those. With
 * gl = gamma * lambda (one float32 multiply) and carry = +0.0f, for k from n_steps - 1 down to 0:
 *   delta  = fmaf(gamma, boot[k], reward[k]) - values[k]      one fma, one subtraction
 *   adv[k] = done[k, e] ? delta : fmaf(gl, carry, delta)
 *   ret[k] = adv[k] + values[k]
 *   carry  = adv[k]
 * No output may alias an input. MACM_E_INVALID: any NULL pointer, a negative size. n_steps = 0 or
 * E N = 0 does nothing.
 */
int macm_gae(const float* reward, const float* values, const float* boot, const uint8_t* done, int32_t n_steps,
             int32_t n_envs, int32_t n_agents, float gamma, float lambda, float* adv, float* ret, void* stream);

/*
 * Parameter gradients of the two MLPs: from dL/dout of every row to dL/dparams, so that a learner's
 * update needs no copy of the net and keeps no per-row activation. The library stays loss-agnostic:
 * the caller turns logits and values into a loss and supplies dout = dL/dlogits [rows, 9] or
 * dL/dvalue [rows]. All arithmetic is float32.
 *   The forward pass is macm_policy_mlp's / macm_value_mlp's as defined above, bit for bit. a_0 is the
 *   float32 input row, a_l the stored (post-relu) activation of hidden layer l; layer l has weights
 *   W_l[in][out], and d_L = dout for the last layer. For each layer, from the last to the first:
 *     gW_l[k][j]    = sum over rows r of a_{l-1}[r][k] * d_l[r][j]
 *     gb_l[j]       = sum over rows r of d_l[r][j]
 *     d_{l-1}[r][k] = (a_{l-1}[r][k] > 0) ? sum_j W_l[k][j] * d_l[r][j] : 0        (l > 1 only)
 *   The relu derivative is taken from the forward's own stored activation, so it is 0 for 0, -0 and
 *   NaN. The association of the sums is not fixed, but the result depends only on the inputs and
 *   `rows`, never on timing: no floating-point atomics, partial sums combined in a fixed order, so two
 *   calls with the same arguments give the same bits.
 *   grad has the layout of params (W then b, layer after layer) and is overwritten, not accumulated;
 *   rows = 0 writes zeros. Non-finite inputs give unspecified results. There is no gradient with
 *   respect to obs.
 * The library holds no state for this: the caller owns the workspace (device memory, 16-byte aligned),
 * of at least macm_mlp_grad_workspace(rows) bytes: enough for either net of any supported shape, a
 * function of rows only, nondecreasing in rows and constant from 2048 * 64 rows on. Its contents after
 * a call are unspecified; two calls in flight at once need a workspace each. Everything is ordered on
 * `stream`. Additive: MACM_ABI_VERSION stays 9.
 * MACM_E_INVALID, with a message and nothing launched: a NULL struct or one outside the supported
 * shapes, reserved != 0, params NULL or misaligned, obs, dout or grad NULL, rows < 0, workspace NULL,
 * misaligned or workspace_bytes too small while rows > 0; macm_mlp_grad_workspace: rows < 0 or bytes NULL.
 */
int macm_mlp_grad_workspace(int64_t rows, int64_t* bytes);
int macm_policy_grad(const macm_policy_mlp* p, const void* obs, int32_t obs_f64, int64_t rows,
                     const float* dlogits /* [rows, 9] */, float* grad /* [n_params] */, void* workspace,
                     int64_t workspace_bytes, void* stream);
int macm_value_grad(const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t rows,
                    const float* dvalues /* [rows] */, float* grad /* [n_params] */, void* workspace,
                    int64_t workspace_bytes, void* stream);

/*
 * The clipped PPO loss on device: from logits and values (or, in macm_ppo_grad, from obs rows) to
 * dL/dlogits, dL/dvalue (dL/dparams) and the statistics, so that an update pass keeps nothing per row
 * but its inputs. The loss-agnostic path above stays; this is one particular loss, defined so that it
 * can be checked. All per-row arithmetic is float64 on the float32 inputs, every operation rounded
 * once, in the association written here; every stored float32 is one rounding of a float64 value.
 * Row r has heads h = 0..2 of MultiDiscrete([3, 3, 3]), z = logits[r], a_h = actions[r][h] (0, 1 or 2):
 *   m_h = max_c z[3h+c]; e_c = exp(z[3h+c] - m_h); S_h = (e_0 + e_1) + e_2; lse_h = m_h + log S_h
 *   lp_hc = z[3h+c] - lse_h; p_hc = e_c / S_h
 *   logp = (lp_0a0 + lp_1a1) + lp_2a2; logp32 = (float)logp       what macm_policy_logp stores
 *   H_h = -((p_h0 lp_h0 + p_h1 lp_h1) + p_h2 lp_h2); H = (H_0 + H_1) + H_2     (macm_policy_logp: (float)H)
 *   ratio = exp((double)logp32 - (double)old_logp)
 *     logp is rounded to float32 before the subtraction, so an old_logp that macm_policy_logp stored
 *     from the same logits gives ratio = 1 exactly; the derivative treats that rounding as the identity.
 *   s1 = ratio adv; s2 = min(max(ratio, 1 - clip), 1 + clip) adv; pl = -min(s1, s2)
 *   g_logp = (s1 <= s2) ? -adv ratio : 0                          a tie takes the unclipped branch
 *   without old_values: vl = (v - ret)^2 / 2; g_v = v - ret
 *   with old_values:    vc = old_v + min(max(v - old_v, -vf_clip), vf_clip); u = (v - ret)^2; c = (vc - ret)^2
 *                       vl = max(u, c) / 2; g_v = (u >= c) ? v - ret : (|v - old_v| <= vf_clip ? vc - ret : 0)
 *   loss = (mean(pl) + vf_coef mean(vl)) - ent_coef mean(H), every mean over the `rows` rows of the call
 *   k = scale / rows (scale NULL: 1)
 *   dlogits[r][3h+c] = (float)(k (g_logp (1[c = a_h] - p_hc) + ent_coef (p_hc (lp_hc + H_h))))
 *   dvalues[r]       = (float)(k (vf_coef g_v))
 * stats is a device double[8]: loss, policy_loss = mean(pl), value_loss = mean(vl), entropy = mean(H),
 * approx_kl = mean((ratio - 1) - log ratio), clip_frac = the share of rows with |ratio - 1| > clip,
 * ratio_max, rows. The sums are float64 and use no atomics: lane-local, then a wave's lanes in lane
 * order, then the partials in a fixed order; the association is a function of `rows` alone, so the same
 * arguments give the same bits on every call and stream. Non-finite inputs give unspecified results.
 *
 * macm_policy_logp: logp [rows] (and entropy [rows] unless NULL) from logits [rows, 9] and actions
 * uint8 [rows, 3]: the old_logp of a trajectory from the logits macm_world_rollout_policy stored.
 * MACM_E_INVALID: logits, actions or logp NULL, rows < 0, a misaligned pointer. rows = 0 writes nothing.
 *
 * macm_ppo_loss: either half may be left out: logits NULL (then actions, old_logp and adv are not read
 * and the policy statistics are 0) or values NULL (likewise ret, old_values and value_loss). old_values
 * NULL selects the unclipped value loss. scale is a DEVICE pointer to one float (an autograd's incoming
 * gradient, handed over without a synchronise) or NULL. dlogits, dvalues and stats may each be NULL:
 * that output is not written. rows = 0 zeros stats and touches nothing else. No output may alias an input.
 *
 * macm_ppo_grad: the loss inside the gradient launch, one launch per net that is given (either may be
 * NULL) plus the reductions: the forward is macm_policy_mlp's / macm_value_mlp's through the last
 * layer, the row's dL/dout is the definition above on those outputs with scale = 1, and everything
 * behind it is macm_policy_grad's / macm_value_grad's, so grad_policy and grad_value have the bits of
 * macm_policy_flock (logits) / macm_value_flock -> macm_ppo_loss -> macm_policy_grad / macm_value_grad
 * while neither the logits nor dL/dlogits exist in memory. Both are overwritten, not accumulated;
 * rows = 0 writes zeros. stats (or NULL) is as above, with the half of a net that is not given 0; its
 * sums are associated per wave of 64 rows, so they may differ from macm_ppo_loss's in the last bits.
 *
 * The caller owns the workspace as for macm_policy_grad: device memory, 16-byte aligned, at least
 * macm_ppo_workspace(rows) bytes (the gradient partials and behind them the stat partials), a
 * nondecreasing function of rows only; its contents after a call are unspecified and two calls in
 * flight need one each. Everything is ordered on `stream`. Additive: MACM_ABI_VERSION stays 9.
 * MACM_E_INVALID, with a message and nothing launched: cfg NULL, clip <= 0, a negative vf_coef or
 * ent_coef, vf_clip <= 0 where old_values is given, reserved != 0, rows < 0, logits and values both
 * NULL (macm_ppo_grad: both nets NULL, a net outside the supported shapes, nets of different in_dim,
 * obs NULL), actions, old_logp or adv NULL where logits (the policy) is given, ret NULL where values
 * (the critic) is given, a gradient output NULL for a net that is given, dlogits (dvalues) without
 * logits (values), a misaligned pointer (float32 arrays 4 bytes, stats 8, workspace 16), workspace
 * NULL or workspace_bytes too small while rows > 0; macm_ppo_workspace: rows < 0 or bytes NULL.
 */
typedef struct macm_ppo_config {
  float clip, vf_coef, ent_coef, vf_clip;
  int32_t reserved[4];
} macm_ppo_config;

int macm_policy_logp(const float* logits /* [rows, 9] */, const uint8_t* actions /* [rows, 3] */, int64_t rows,
                     float* logp /* [rows] */, float* entropy /* [rows] or NULL */, void* stream);
int macm_ppo_workspace(int64_t rows, int64_t* bytes);
int macm_ppo_loss(const macm_ppo_config* cfg, int64_t rows, const float* logits, const uint8_t* actions,
                  const float* old_logp, const float* adv, const float* values, const float* ret,
                  const float* old_values, const float* scale, float* dlogits, float* dvalues, double* stats,
                  void* workspace, int64_t workspace_bytes, void* stream);
int macm_ppo_grad(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs,
                  int32_t obs_f64, int64_t rows, const uint8_t* actions, const float* old_logp, const float* adv,
                  const float* ret, const float* old_values, float* grad_policy, float* grad_value, double* stats,
                  void* workspace, int64_t workspace_bytes, void* stream);

/*
 * PPO updates over shuffled minibatches with normalised advantages: macm_ppo_grad reading its rows through
 * an index list, and the moments of a minibatch's advantages from a deterministic device reduction.
 *
 * macm_ppo_grad_rows is macm_ppo_grad with three more arguments. Position r of the call, 0 <= r < rows,
 * reads source row s = index[r] (int32 [rows]; index NULL: s = r) of obs, actions, old_logp, adv, ret and
 * old_values, which hold n_src rows each; repeats and any order are allowed. With adv_norm (a DEVICE
 * double[2] {mean, rstd}, read with no synchronise) the row's advantage is
 *   (float)(((double)adv[s] - adv_norm[0]) * adv_norm[1])
 * one subtraction and one multiplication in float64, one rounding to float32. Everything else is
 * macm_ppo_grad's definition in terms of the position: k = 1 / rows, the means over rows, the tile and
 * the wave of a position, the partials, the reductions and stats, so the association of every sum is a
 * function of rows alone and never of the index values: the outputs have the bits of macm_ppo_grad
 * called on contiguous gathered (and normalised) copies of the inputs. A position whose index is outside
 * [0, n_src) is treated as a lane past rows: nothing of it is loaded, it adds exact zeros to the
 * gradients and nothing to the stats, while k stays 1 / rows and stats[7] stays rows; no index value
 * makes the library read outside the caller's arrays. With index NULL n_src is checked and not read.
 * The workspace is macm_ppo_workspace(rows) bytes, rows being the index length.
 * MACM_E_INVALID, with a message and nothing launched: everything macm_ppo_grad refuses; n_src < 0 or
 * n_src > 2^31 - 1; index and adv_norm both NULL (that call is macm_ppo_grad: there is one way to do
 * each thing); index not 4-byte or adv_norm not 8-byte aligned.
 *
 * macm_adv_moments: with x_r = (double)x[index ? index[r] : r] over the n positions whose source row
 * is in [0, n_src) (index NULL: all rows of them; n_src is checked and not read),
 *   mean = sum x_r / n (n = 0: 0); S2 = sum (x_r - mean)^2, a second pass with that mean
 *   var = n > 1 ? S2 / (n - 1) : 0 (unbiased: torch's tensor.std()); std = sqrt(var); rstd = 1 / (std + eps)
 *   out = {mean, rstd, std, (double)n}: a device double[4], and as it stands a valid adv_norm
 * so that macm_ppo_grad_rows behind it computes (adv - mean) / (std + eps) of the minibatch with no
 * synchronise between. The sums are float64 with no atomics: lane-local, a wave's lanes in lane order,
 * the partials in a fixed order; their association is a function of rows alone, so the same arguments
 * give the same bits on every call and stream. Four small launches ordered on `stream`. rows = 0
 * writes {0, 1 / eps, 0, 0}. The workspace is the caller's as above; macm_ppo_workspace(rows) bytes
 * suffice and are what is asked for. MACM_E_INVALID: x or out NULL, rows < 0, n_src outside
 * [0, 2^31 - 1], eps negative or not finite, x or index not 4-byte, out not 8-byte aligned, workspace
 * NULL, not 16-byte aligned or workspace_bytes too small while rows > 0. Additive: MACM_ABI_VERSION stays 9.
 */
int macm_ppo_grad_rows(const macm_ppo_config* cfg, const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs,
                       int32_t obs_f64, int64_t rows, const int32_t* index /* [rows] or NULL */, int64_t n_src,
                       const double* adv_norm /* device {mean, rstd} or NULL */, const uint8_t* actions,
                       const float* old_logp, const float* adv, const float* ret, const float* old_values,
                       float* grad_policy, float* grad_value, double* stats, void* workspace, int64_t workspace_bytes,
                       void* stream);
int macm_adv_moments(const float* x, const int32_t* index /* [rows] or NULL */, int64_t n_src, int64_t rows, double eps,
                     double* out /* device double[4] */, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The PPO update on device: Adam with global-norm clipping, a KL gate and a non-finite guard in one launch
 * (macm_ppo_adam), and any number of minibatches (moments -> fused gradients -> step) enqueued by one call
 * with nothing synchronising (macm_ppo_update).
 *
 * macm_ppo_adam updates the params of both nets in place from grad_policy [n_p] and grad_value [n_c] (n_p,
 * n_c: the nets' parameter counts, at most 1,577 each; a net that is NULL has n = 0). One workgroup of 256
 * threads; the elements are the concatenation policy then critic, j = 0 .. n_p + n_c - 1, and element j
 * belongs to thread j mod 256. All arithmetic is float64 on the float32 inputs, every operation rounded
 * once, in the association written here, with + - * / sqrt only; what is stored as float32 is one rounding
 * of a float64.
 *
 * state is device memory, 8-byte aligned, macm_ppo_adam_state_bytes(p, c) = 64 + 8 (n_p + n_c) bytes:
 *   double head[8]; float m_p[n_p]; float v_p[n_p]; float m_c[n_c]; float v_c[n_c]
 *   head[0] t, the steps applied         head[4] the last gradient norm
 *   head[1] beta1^t                      head[5] the last clip coefficient
 *   head[2] beta2^t                      head[6] the steps skipped for a non-finite norm
 *   head[3] stopped, 0 or 1              head[7] 0
 * An all-zero state is a fresh optimiser: with t = 0 both powers are taken as 1. The powers are running
 * products (p1' = p1 beta1), never a pow. The state belongs to one pair of net shapes.
 *
 * One call, in this order:
 *   1. head[3] != 0: nothing is written at all (a stopped optimiser stays as it is until the caller
 *      writes 0.0 to head[3]).
 *   2. stats given and target_kl > 0 and !(stats[4] <= target_kl): head[3] = 1, nothing else is written.
 *      stats[4] is approx_kl of macm_ppo_grad's stats; a NaN stops.
 *   3. s_i (thread i) = the sum over its elements j = i, i + 256, ... in ascending j, from 0, of
 *      (double)g_j (double)g_j; then s[i] += s[i + d] for i < d, d = 128, 64, ..., 1; norm = sqrt(s[0]).
 *      norm not finite: head[6] += 1, head[4] = norm, nothing else is written.
 *   4. coef = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1    (torch's clip_grad_norm_)
 *   5. p1 = t == 0 ? 1 : head[1]; p2 likewise; p1' = p1 beta1; p2' = p2 beta2; per element
 *        g = (double)grad coef
 *        m' = (float)(beta1 (double)m + (1 - beta1) g)
 *        v' = (float)(beta2 (double)v + (1 - beta2) (g g))
 *        param' = (float)((double)param - lr (((double)m' / (1 - p1')) / (sqrt((double)v' / (1 - p2')) + eps)))
 *      with 1 - beta formed on the host in double.
 *   6. head[0] = t + 1, head[1] = p1', head[2] = p2', head[4] = norm, head[5] = coef.
 * The config is passed by value on every call: a schedule is the caller changing lr. The params are written
 * in place, and the next launch on the stream reads them from memory: stream order is the only ordering
 * needed. The gradients are not modified. (macm_policy_mlp and macm_value_mlp declare params const because
 * every other call only reads them; this one writes through that pointer, so the memory must be writable.)
 * MACM_E_INVALID, with a message and nothing launched: opt NULL, both nets NULL, a net outside the supported
 * shapes, a gradient NULL for a net that is given, state NULL, a misaligned pointer (gradients 4 bytes, stats
 * and state 8), state_bytes below macm_ppo_adam_state_bytes, reserved != 0, lr negative or not finite, a beta
 * outside [0, 1), eps <= 0 or not finite, max_grad_norm or target_kl negative or not finite, target_kl > 0
 * without stats or without the policy.
 *
 * macm_ppo_update is a host loop over the launches of macm_adv_moments, macm_ppo_grad_rows and
 * macm_ppo_adam: for minibatch i = 0 .. n_minibatches - 1, with index[i] (a device int32 [rows[i]]; index
 * and rows themselves are HOST arrays) naming source rows of the n_src-row arrays,
 *   the moments of adv at index[i] (if normalize_adv and the policy is given; eps = adv_eps),
 *   the fused gradient launch of each net that is given, with those moments as adv_norm,
 *   the statistics into stats[8 i .. 8 i + 7] (stats: device double [n_minibatches, 8], or NULL),
 *   the step, gated by that row of statistics,
 * all on `stream`, nothing synchronised, nothing allocated; the moments, the gradients and (stats NULL) the
 * statistics live in the workspace and are reused from minibatch to minibatch, the launches being ordered.
 * The results have the bits of the same sequence of single calls. A minibatch of 0 rows is skipped whole:
 * its stats row is zeroed and no step is taken (a zero gradient would still move the params on momentum).
 * After a KL stop the remaining minibatches' gradient launches still run and their stats rows are written;
 * they describe the unchanged params. That waste is bounded by the call; ending early on the host would
 * need the very synchronise this entry point exists to avoid. Epochs are the caller's notion: two epochs
 * are the two epochs' minibatches in one list. The workspace is the caller's, device memory, 16-byte
 * aligned, macm_ppo_update_workspace(max_rows) bytes for the largest rows[i] (nondecreasing in max_rows).
 * MACM_E_INVALID, with a message and nothing launched: everything macm_ppo_grad_rows and macm_ppo_adam
 * refuse, n_minibatches < 0, index or rows NULL while n_minibatches > 0, a rows[i] < 0, an index[i] NULL or
 * misaligned while rows[i] > 0, adv_eps negative or not finite, workspace NULL or too small.
 * Additive: no struct changed, MACM_ABI_VERSION stays 9.
 */
typedef struct macm_adam_config {
  double lr, beta1, beta2, eps;   /* by value on every call: a schedule is the caller changing lr */
  double max_grad_norm;           /* 0: no clipping */
  double target_kl;               /* 0: no gate; compared as given with stats[4] (a user of the 1.5 x convention passes 1.5 x) */
  int32_t reserved[4];            /* 0 */
} macm_adam_config;

int macm_ppo_adam_state_bytes(const macm_policy_mlp* p, const macm_value_mlp* c, int64_t* bytes);
int macm_ppo_adam(const macm_adam_config* opt, const macm_policy_mlp* p, const macm_value_mlp* c,
                  const float* grad_policy, const float* grad_value, const double* stats /* [8] or NULL */,
                  void* state, int64_t state_bytes, void* stream);

int macm_ppo_update_workspace(int64_t max_rows, int64_t* bytes);
int macm_ppo_update(const macm_ppo_config* cfg, const macm_adam_config* opt,
                    const macm_policy_mlp* p, const macm_value_mlp* c, const void* obs, int32_t obs_f64, int64_t n_src,
                    const uint8_t* actions, const float* old_logp, const float* adv, const float* ret,
                    const float* old_values, int32_t n_minibatches,
                    const int32_t* const* index /* host array of device pointers */,
                    const int64_t* rows /* host array */, int32_t normalize_adv, double adv_eps,
                    void* state, int64_t state_bytes, double* stats /* device [n_minibatches, 8] or NULL */,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* Observation of the current state without stepping (Flock.get_obs, mvmnt.py:181-222). */
int macm_world_observe(macm_world* w, const macm_outputs* out, void* stream);

/*
 * Copy state out / in (synchronous w.r.t. `stream`). set_state validates the contact lists
 * it is given (when contact_count is non-NULL): 0 <= count <= min(C, contact_stride) and, for
 * every entry below the count, a < b < N, checked on the device after staging the lists into the
 * world's spare list buffer; otherwise MACM_E_INVALID and nothing is copied. contact_count and
 * contact_ab must be given together (contact_imp NULL: zero impulses). Clears the status bits.
 */
int macm_world_get_state(macm_world* w, const macm_state* dst, void* stream);
int macm_world_set_state(macm_world* w, const macm_state* src, void* stream);

/* OR over envs of the per-env status bits (synchronises `stream`). */
int macm_world_status(macm_world* w, int32_t* status_or, void* stream);

/*
 * Per-world counters, accumulated on device by every step (synchronises `stream`):
 *   out[0] agent-steps, out[1] collided agent-steps, out[2] positive-reward
 *   agent-steps, out[3] env-steps with done set. Used for the RCCL all-reduce
 *   in multi-GPU runs. reset_counters zeroes them.
 */
int macm_world_counters(macm_world* w, int64_t out[4], void* stream);
int macm_world_reset_counters(macm_world* w, void* stream);  /* also zeroes the reward sums */

/*
 * The rewards' sum (Σ of get_rewards' values, mvmnt.py:160-179), in float64 and
 * in a fixed order so that it is bit-stable (ABI 8): each step's float32 rewards are summed as
 * float64 pairwise over the agent slots 0 .. P-1 (P = 64 * 2^ceil(log2(ceil(N / 64))), +0.0 past N:
 * ((r0 + r1) + (r2 + r3)) + ...), that sum is added to the env's total in step order, and `total`
 * is the envs' totals summed in env order from +0.0. Binary rewards (-1, 0, +1) make every partial sum
 * an exact integer, so a binary world's env total is read as counter 2 - counter 1 (the same bits; the
 * kernels accumulate the float64 sums for linear rewards only). per_env: host double [E] or NULL; total: host
 * double or NULL (not both NULL). Accumulated by every step since creation or reset_counters;
 * synchronises `stream`. Multi-GPU: gather the per-env totals and sum them in global env order
 * (gym_macm.dist.reduce_reward_sums), which gives the single-process total at any rank count.
 */
int macm_world_reward_sums(macm_world* w, double* per_env, double* total, void* stream);

/* Env-steps taken by the spill step since creation (dense worlds; synchronises `stream`). */
int macm_world_spilled(macm_world* w, int64_t* env_steps, void* stream);

/* Test hooks: MACM_DEBUG_* flags (0 = product behaviour). */
int macm_world_set_debug(macm_world* w, int32_t flags);

/* ---- TDM (gym_macm:cm-tdm-v0, combat.py:57-264) -------------------------- */

typedef struct macm_tdm macm_tdm;

/* combatSettings / Agent defaults (settings.py:149-177, combat.py:13-29), n_agents=[1,1]. */
int macm_tdm_config_default(macm_tdm_config* cfg);

/*
 * Create E TDM envs (N = sum(team_size) <= 4096 agents; MACM_E_UNSUPPORTED above). Replaces
 * TDM.__init__'s world + body creation (combat.py:61-102). State is undefined until reset/place.
 * N <= 64: one wave per env (the fast kernel, its spill step for crowded envs); N > 64: one
 * workgroup per env (tdm_step_wg.hip: the action loop, then the spill step's physics with its HBM
 * working set for every env; macm_tdm_spilled counts every such env-step). Rollouts on the
 * workgroup path are one launch per step (and the bots kernel's), with the same results.
 */
int macm_tdm_create(const macm_tdm_config* cfg, int32_t n_envs, int32_t device, macm_tdm** out);
int macm_tdm_destroy(macm_tdm* w);

/*
 * Initialise every env as TDM.__init__ after random.seed(seed + env_offset + e):
 * per agent in team order x = random()*(team + width/2), y = random()*height,
 * angle = uniform(-1, 1)*pi (combat.py:80-95). Writes the initial obs into `out`.
 */
int macm_tdm_reset(macm_tdm* w, uint64_t seed, int64_t env_offset, const macm_tdm_outputs* out, void* stream);

/* As reset with caller-drawn poses: pos [E, N, 2] float32, angle [E, N] float32. */
int macm_tdm_place(macm_tdm* w, const void* pos, const void* angle, const macm_tdm_outputs* out, void* stream);

/*
 * As macm_world_reset_envs for TDM: the masked envs draw new spawn poses from
 * their streams (combat.py:234-245 draw order), every agent revived with
 * init_health, zero cooldowns, a fresh listener, winner -1.
 */
int macm_tdm_reset_envs(macm_tdm* w, const uint8_t* env_mask, const macm_tdm_outputs* out, void* stream);

/*
 * As macm_world_set_autoreset for TDM: an env that ends (a team wiped out, or the time limit) is
 * reset as by macm_tdm_reset_envs before its next step, in macm_tdm_step and inside every rollout.
 * The outputs of such a step keep the terminal done (1), winner, health and alive as the step
 * wrote them (the trajectory shows who won); obs and mask of the reset envs are the new episode's.
 * Rollouts of such a world observe inside the step: macm_tdm_launch_flags reports 0 and
 * macm_tdm_reserve is a no-op. Status, placed worlds and NULL as for macm_world_set_autoreset.
 * Additive: no struct changed, MACM_ABI_VERSION stays 9.
 * The obs and mask that the reset overwrites are kept where macm_tdm_set_final_outputs says.
 */
int macm_tdm_set_autoreset(macm_tdm* w, int32_t on);

/* As macm_world_set_final_outputs (macm_final_outputs: obs, mask, length, ends; nbr_id ignored). */
int macm_tdm_set_final_outputs(macm_tdm* w, const macm_final_outputs* fin);

/*
 * Combat events: who damaged whom, per agent and per step. The reference's TDM has no reward
 * (get_rewards is `pass`) and a health trajectory does not say whose attack did the damage; the
 * ordered listener update inside the step is the only place that knows, and this exports it.
 *
 * hit_id[e, i] of one step is the env-local index j of the body whose health agent i's attack
 * reduced in that step, or -1: i was dead at the step's start, its attack bit was 0, its
 * cooldown_atk was above 0, or its attack damaged nobody (fresh_raycast: the ray hit no one; the
 * literal listener: nothing has been hit yet in this episode). With the literal listener j is the
 * listener's body after i's cast: the body i's ray hit, or else the last body any earlier cast of
 * the episode hit, which may be an ally, i itself or a body that is already dead.
 *
 * Every step that writes an env's `health` output also writes all N entries of the env's row; an
 * env left unstepped (MACM_ST_SPILL_WAIT) keeps its row. macm_tdm_reset, _place, _reset_envs,
 * _observe and the reset of an autoreset world never write events: a terminal step's row keeps what
 * the step wrote, as health, alive and winner do.
 * macm_tdm_step, _rollout and _rollout_bots write row 0 (rollouts: the last step's row remains);
 * macm_tdm_rollout_traj and _rollout_bots_traj write step k into row k and return MACM_E_INVALID,
 * stepping nothing, when n_steps > rows.
 *
 * A registration, as macm_tdm_set_final_outputs: the world keeps a copy of the struct, not of the
 * buffer, which must stay valid until the registration is replaced or cleared (ev NULL, or hit_id
 * NULL) or the world is destroyed. MACM_E_INVALID with a message, nothing changed: a NULL world, a
 * misaligned hit_id, rows < 1 with a non-NULL hit_id. With nothing registered every call launches
 * the kernels it launched before events existed. Additive: no struct changed, MACM_ABI_VERSION stays 9.
 */
typedef struct macm_tdm_events {
  int32_t* hit_id; /* [rows, E, N]; device or host-mapped pointer, 4-byte aligned; NULL = none */
  int32_t rows;    /* rows the caller allocated (>= 1)                                         */
} macm_tdm_events;
int macm_tdm_set_events(macm_tdm* w, const macm_tdm_events* ev);

/*
 * One TDM.step for all E envs (combat.py:104-184). actions: device uint8
 * [E, N, 4] (MultiDiscrete([3,3,3,2]): forward, lateral, rotation, attack);
 * rows of dead agents are ignored. An env with more than 256 touching contacts or a body touching
 * more than 16 others (a crowded small world) is stepped by the spill step (HBM working set,
 * every pair; after its actions, casts and deaths) with the same results. MACM_E_INVALID with
 * validate_actions; MACM_E_OVERFLOW only after a SPILL_WAIT (pooled working set).
 */
int macm_tdm_step(macm_tdm* w, const void* actions, const macm_tdm_outputs* out, void* stream);

/*
 * As macm_world_rollout for TDM: actions [n_steps, E, N, 4] uint8, one launch. With
 * validate_actions every row is checked, the dead agents' rows included (deaths within the
 * rollout are not known when the check runs).
 */
int macm_tdm_rollout(macm_tdm* w, const void* actions, int32_t n_steps, const macm_tdm_outputs* out, void* stream);

/* The closed loop `step -> bots.combat -> step` in one launch (as macm_world_rollout_bots);
 * actions uint8 [E, N, 4] in/out, out->obs and out->mask must be set. */
int macm_tdm_rollout_bots(macm_tdm* w, uint8_t* actions, int32_t n_steps, const macm_tdm_outputs* out, void* stream);

/* Trajectory forms of the two above (as macm_world_rollout_traj): obs [n_steps, E, N, N-1, 4],
 * mask [n_steps, E, N, N-1], health / alive [n_steps, E, N], done / winner [n_steps, E]; bots:
 * actions [n_steps + 1, E, N, 4]. */
int macm_tdm_rollout_traj(macm_tdm* w, const void* actions, int32_t n_steps, const macm_tdm_outputs* traj,
                          void* stream);
int macm_tdm_rollout_bots_traj(macm_tdm* w, uint8_t* actions, int32_t n_steps, const macm_tdm_outputs* traj,
                               void* stream);

/*
 * A learned policy as the actor of TDM's closed loop: a permutation-invariant float32 net over the
 * [N-1, 4] observation slots of an agent, in the place of the scripted bot, with a team mask so that
 * one side learns against bots.combat on the other. Defined so that it can be checked bit for bit; all
 * arithmetic float32, the conventions of macm_policy_mlp (explicit fmaf chains with k ascending and one
 * rounding per step; relu(v) = v > 0 ? v : +0.0f). For agent i of an env with N agents, with its obs row
 * o[N-1][4] as stored (float64 obs round to nearest), its mask row m[N-1] and its health h (the double
 * of macm_tdm_outputs.health rounded to float32):
 *   encoder for every slot k with m[k] != 0: e_k[j] = relu(b1[j] + sum_q W1[q][j] o[k][q]), q = 0..3 ascending;
 *   pool    g[j] = +0.0f, then g[j] = e_k[j] > g[j] ? e_k[j] : g[j] over the live slots. After the relu no e
 *           is NaN or negative, so the pooled value does not depend on the order of the slots; a row with
 *           no live slot (a dead agent, the last one standing) pools to zeros and still yields an action;
 *           what a masked slot holds (NaN, inf, -0) changes nothing;
 *   trunk   u = (g[0..H-1], h); t[j] = relu(b2[j] + sum_k W2[k][j] u[k]), k = 0..H ascending (the health
 *           is input k = H);
 *   head    z[c] = b3[c] + sum_k W3[k][c] t[k]: 11 logits of MultiDiscrete([3, 3, 3, 2]), heads 0..2 at
 *           z[3h + c], head 3 (attack) at z[9] and z[10];
 *   action  the rule of macm_policy_mlp, word for word, per head: z[c] + noise[c] if noise is given (one
 *           float32 add), then the lowest c with the largest value by `>` from -inf. 4 bytes: forward,
 *           lateral, rotation, attack.
 *   params: device float32, 16-byte aligned, row-major [in][out]:
 *           W1[4][H], b1[H], W2[H+1][H], b2[H], W3[H][11], b3[11] (1,611 floats at H = 32).
 * hidden (H) is 16 or 32, reserved 0. The caller supplies the noise. Out of scope: a critic, an in-launch
 * draw, continuous actions. Additive: MACM_ABI_VERSION stays 9.
 */
typedef struct macm_tdm_policy {
  int32_t hidden;
  int32_t reserved[3];
  const float* params;
} macm_tdm_policy;

/*
 * The policy's decision for `rows` agent rows (rows = E * n_agents: obs [rows, N-1, 4] float32 or float64
 * as obs_f64 and 16-byte aligned, mask [rows, N-1], health [rows] float64), as macm_bots_combat is for the
 * bot. agents: uint8 [n_agents] on the device, or NULL (every agent); where agents[row % n_agents] == 0
 * the row's action bytes and logits row are left untouched, so a caller can run the bot first and the
 * policy over it. noise [rows, 11] or NULL; actions uint8 [rows, 4] (4-byte aligned); logits [rows, 11] or
 * NULL. MACM_E_INVALID, nothing launched: p NULL, hidden outside 16 / 32, reserved != 0, params NULL or
 * misaligned, obs / mask / health / actions NULL or misaligned, n_agents < 2, rows < 0 or no multiple of
 * n_agents.
 */
int macm_policy_tdm(const macm_tdm_policy* p, const void* obs, const uint8_t* mask, const double* health,
                    int32_t obs_f64, int32_t n_agents, int64_t rows, const uint8_t* agents, const float* noise,
                    uint8_t* actions, float* logits, void* stream);

/*
 * Parameter gradients of the set policy: from dL/dlogits of every agent row to dL/dparams, as
 * macm_policy_grad is for the MLP, so that a TDM learner's update keeps no per-slot activation. The
 * arguments before dlogits are macm_policy_tdm's. All arithmetic is float32.
 *   The forward pass is macm_tdm_policy's as defined above, bit for bit: o (the slots as the forward read
 *   them: a float64 obs rounded to float32), e_k, g, u = (g, float32(health)), t. With d3 = dlogits of the
 *   row, and every relu derivative taken from the forward's own stored activation (0 for 0, -0 and NaN):
 *     gW3[k][c] = sum over rows r of t[r][k] * d3[r][c]              gb3[c] = sum_r d3[r][c]
 *     d2[r][j]  = (t[r][j] > 0) ? sum_c W3[j][c] * d3[r][c] : 0
 *     gW2[k][j] = sum_r u[r][k] * d2[r][j] for k = 0..H (row H is the health row)
 *     gb2[j]    = sum_r d2[r][j]
 *     dg[r][j]  = (g[r][j] > 0) ? sum_i W2[j][i] * d2[r][i] : 0      (the health gets no gradient)
 *   The pool: unit j of row r has a winner k*(r, j), the lowest live slot k with e_k[j] == g[j], and only
 *   when g[j] > 0: the slot at which the forward's `e > g ? e : g` scan last changed g[j]. A unit with
 *   g[j] == 0 (the empty set, every live e <= 0, NaN pre-activations) has no winner: it contributes exact
 *   zeros to layer 1 and no slot is read for it. A masked slot is never a winner and never read into a
 *   gradient, whatever it holds. Over the (r, j) that have a winner:
 *     gW1[q][j] = sum_r o[r][k*][q] * dg[r][j]                       gb1[j] = sum_r dg[r][j]
 *   Where agents[row % n_agents] == 0 the row takes no part: its obs, mask, health and dlogits are not
 *   read. There is no gradient with respect to obs or health.
 *   grad has the layout of params and is overwritten, not accumulated; rows = 0 writes zeros. Non-finite
 *   values in live slots give unspecified results. The association of the sums is the kernel's and a
 *   function of `rows` alone: no floating-point atomics, partial sums combined in a fixed order, so two
 *   calls with the same arguments give the same bits on any stream.
 * The caller owns the workspace (device memory, 16-byte aligned) of at least macm_tdm_grad_workspace(rows)
 * bytes: a function of rows only, nondecreasing in rows and constant from 2048 * 64 rows on. Its contents
 * after a call are unspecified; two calls in flight at once need a workspace each. Everything is ordered
 * on `stream`. Additive: MACM_ABI_VERSION stays 9.
 * MACM_E_INVALID, with a message and nothing launched (decided before any device call): everything
 * macm_policy_tdm refuses of p, obs, mask, health, n_agents and rows; dlogits or grad NULL; workspace NULL,
 * misaligned or workspace_bytes too small while rows > 0; macm_tdm_grad_workspace: rows < 0 or bytes NULL.
 */
int macm_tdm_grad_workspace(int64_t rows, int64_t* bytes);
int macm_tdm_policy_grad(const macm_tdm_policy* p, const void* obs, const uint8_t* mask, const double* health,
                         int32_t obs_f64, int32_t n_agents, int64_t rows, const uint8_t* agents,
                         const float* dlogits /* [rows, 11] */, float* grad /* [n_params] */, void* workspace,
                         int64_t workspace_bytes, void* stream);

/*
 * Registers the policy of macm_tdm_rollout_policy, as macm_world_set_policy: the world keeps the struct,
 * not the params buffer; a later launch reads params the learner overwrote in place. p NULL clears the
 * registration (team_mask is ignored). Bit t of team_mask gives team t to the policy; the agents of the
 * other teams keep bots.combat. MACM_E_INVALID, nothing changed: a NULL world, a struct the one-shot
 * call would refuse, team_mask 0 or with a bit at or above n_teams. Synchronises the device (the team
 * mask is copied to it).
 */
int macm_tdm_set_policy(macm_tdm* w, const macm_tdm_policy* p, uint32_t team_mask);

/*
 * n_steps of the closed loop `step -> actor -> step`, as macm_tdm_rollout_bots / _bots_traj with the
 * registered policy as the actor of its teams: one launch on the wave path (N <= 64); on the workgroup
 * path the launches of macm_tdm_step, the bots kernel and macm_policy_tdm on the caller's stream.
 *   actions: [E, N, 4] in and out; trajectory form [n_steps + 1, E, N, 4], row 0 given, step k writes row k + 1.
 *   noise:   [n_steps, E, N, 11] or NULL; row k is used for the decision taken after step k.
 *   logits:  [E, N, 11] (the last step's remain), trajectory form [n_steps, E, N, 11], or NULL; the rows of
 *            bot-driven agents are not written.
 * out->obs, out->mask and out->health must be set. With autoreset on, the agents of a reset env decide on
 * its new initial obs and mask and on init_health (the step's health output keeps the terminal health),
 * as the per-step loop (macm_tdm_step, macm_tdm_reset_envs(done), macm_bots_combat, macm_policy_tdm) sees
 * them. Events and final outputs as in every other form. MACM_E_INVALID without a registered policy.
 * n_steps = 0 does nothing. Same results as n_steps of the per-step loop, bit for bit.
 */
int macm_tdm_rollout_policy(macm_tdm* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                            const macm_tdm_outputs* out, void* stream);
int macm_tdm_rollout_policy_traj(macm_tdm* w, uint8_t* actions, int32_t n_steps, const float* noise, float* logits,
                                 const macm_tdm_outputs* traj, void* stream);

/* TDM.get_obs of the current state without stepping. */
int macm_tdm_observe(macm_tdm* w, const macm_tdm_outputs* out, void* stream);

int macm_tdm_get_state(macm_tdm* w, const macm_tdm_state* dst, void* stream);
int macm_tdm_set_state(macm_tdm* w, const macm_tdm_state* src, void* stream);
int macm_tdm_status(macm_tdm* w, int32_t* status_or, void* stream);

/* out[0] alive agent-steps, out[1] melee attacks, out[2] deaths, out[3] env-steps with done. */
int macm_tdm_counters(macm_tdm* w, int64_t out[4], void* stream);

/* Env-steps taken by the spill step since creation (ABI 6). */
int macm_tdm_spilled(macm_tdm* w, int64_t* env_steps, void* stream);

/* MACM_LAUNCH_* of the next macm_tdm_step / rollout (not the closed loop) (ABI 9). */
int macm_tdm_launch_flags(const macm_tdm* w);

/* Allocates ahead what trajectory rollouts of up to n_steps steps need (the tail observation's pose
 * snapshots, MACM_LAUNCH_TAIL_OBS), so that the rollout itself does not reallocate (a reallocation
 * synchronises its stream); optional (a rollout grows what it needs). Synchronises `stream`. */
int macm_tdm_reserve(macm_tdm* w, int32_t n_steps, void* stream);

/* Test hooks: MACM_DEBUG_FORCE_SPILL, MACM_DEBUG_SPILL_POOL (ABI 6). */
int macm_tdm_set_debug(macm_tdm* w, int32_t flags);

/* ---- scripted actors on the device (test_scripts/bots.py) ------------------
 * Read an observation tensor written by a step and write the next actions, so a
 * closed-loop rollout stays in HBM. Device pointers; asynchronous on `stream`.
 * With float64 obs the decisions equal the reference bots' on the same obs.
 */

/* bots.flock (bots.py:37-61) on Flock obs [rows, obs_dim] (4 polar, 6 cartesian);
 * actions [rows, 3] uint8. rows = E * N. */
int macm_bots_flock(const void* obs, int32_t obs_f64, int32_t obs_dim, int64_t rows, uint8_t* actions,
                    void* stream);

/* bots.combat (bots.py:3-16) on TDM obs [rows, N-1, 4] + mask [rows, N-1];
 * actions [rows, 4] uint8 (rows of dead agents get the idle action). rows = E * N. */
int macm_bots_combat(const void* obs, const uint8_t* mask, int32_t obs_f64, int32_t n_agents, int64_t rows,
                     uint8_t* actions, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MACM_H */
