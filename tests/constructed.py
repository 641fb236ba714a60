"""Constructed states for both worlds (tests/ only): injection into the oracle and the HIP world,
filler parking, and the scenarios that reach the step's branches a random rollout never takes
(the translation clamp, the degenerate contact normal, Normalize's early return, the clamped
position correction, and the boundaries of the melee ray cast).

A scenario is a list of small groups of bodies given relative to the group's origin. A layout puts
one group into each env (N = 4) or stacks several in one env, far enough apart that they never
meet, and parks the remaining bodies on a lattice away from all of them."""
import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)      # b2_epsilon = FLT_EPSILON = 2^-23
AABB_EXT = F(0.1)                      # b2_aabbExtension
IDLE = (1, 1, 1)                       # Flock's no-op action
FORWARD = (2, 1, 1)


def step_f32(x, k):
    """The float32 k places above (k > 0) or below (k < 0) float32(x)."""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf), dtype=np.float32)
    return x


def fresh_fat(p, radius=0.5):
    """The fat AABBs of bodies created at p [..., 2]: (p -+ r) -+ b2_aabbExtension, in float32."""
    p = np.asarray(p, np.float32)
    r = F(radius)
    return np.concatenate([(p - r) - AABB_EXT, (p + r) + AABB_EXT], -1)


def fat_pairs(fat, active=None):
    """The pairs (a < b) of overlapping fat AABBs [N, 4] in FindNewContacts order (a descending, then
    b descending), among the active bodies."""
    N = fat.shape[0]
    lo, hi = fat[:, :2], fat[:, 2:]
    ov = ~((lo[None, :, 0] > hi[:, None, 0]) | (lo[None, :, 1] > hi[:, None, 1]) |
           (lo[:, None, 0] > hi[None, :, 0]) | (lo[:, None, 1] > hi[None, :, 1]))
    if active is not None:
        on = np.asarray(active, bool)
        ov &= on[:, None] & on[None, :]
    return [(a, int(b)) for a in range(N - 1, -1, -1) for b in np.nonzero(ov[a, a + 1:])[0][::-1] + a + 1]


def _write_bodies(st, e, pos, vel, angle, radius, fat_fn, active, C):
    p = pos[e].astype(np.float32)
    st["pos"][e] = p
    st["vel"][e] = 0.0 if vel is None else vel[e].astype(np.float32)
    st["sleep"][e] = 0.0
    if angle is not None:
        st["angle"][e] = angle[e].astype(np.float32)
    st["fat"][e] = fresh_fat(p, radius)
    if fat_fn is not None:
        fat_fn(e, st["fat"][e])
    pairs = fat_pairs(st["fat"][e], active)
    assert len(pairs) <= C
    st["contact_count"][e] = len(pairs)
    st["contact_ab"][e] = 0
    if pairs:
        st["contact_ab"][e, :len(pairs)] = [a | (b << 16) for a, b in pairs]
    st["contact_imp"][e] = 0.0


def inject(vec, orc, pos, fat_fn=None, vel=None, angle=None, radius=0.5, capacity=None):
    """Place bodies at pos [E, N, 2] (velocities vel [E, N, 2] or zero, angles kept unless given,
    fresh fat AABBs of `radius` — or fat_fn(e, fat) — and the pair list of the overlapping fat AABBs
    in FindNewContacts order) in both worlds. vec = None: the oracle alone."""
    import torch
    E, N = pos.shape[:2]
    C = vec.world.C if vec is not None else (capacity or N * (N - 1) // 2)
    # one step first: the oracle's first Step runs the pending FindNewContacts of the freshly
    # created fixtures (Box2D's e_newFixture), which would rebuild the injected fat AABBs
    idle = np.ones((E, N, 3), np.uint8)
    orc.step(idle)
    if vec is not None:
        vec.step(torch.from_numpy(idle).cuda())
    st = orc.get_state(C)
    for e in range(E):
        _write_bodies(st, e, pos, vel, angle, radius, fat_fn, None, C)
    orc.set_state(st)
    if vec is not None:
        vec.set_state(st)


def inject_tdm(w, orc, pos, angle, alive=None, health=None, radius=0.5):
    """inject's TDM twin: poses, zero velocities, fresh fat AABBs and their pair list (contact
    capacity N(N-1)/2), with alive and health [E, N] if given; a dead body is inactive and in no
    pair. Through OracleTDM.get_state / set_state and TdmWorld.set_state; w = None: the oracle alone."""
    import torch
    E, N = pos.shape[:2]
    C = N * (N - 1) // 2
    idle = np.ones((E, N, 4), np.uint8)
    idle[..., 3] = 0
    orc.step(idle)
    if w is not None:
        w.step(torch.from_numpy(idle).cuda())
    st = orc.get_state()
    for e in range(E):
        _write_bodies(st, e, pos, None, angle, radius, None, None if alive is None else alive[e], C)
    if alive is not None:
        st["alive"][:] = alive
    if health is not None:
        st["health"][:] = health
    orc.set_state(st)
    if w is not None:
        w.set_state(st)


def park_fillers(n, keep_out, rays=(), spacing=1.5, clear=5.0, radius=0.5, cols=40):
    """n parking places on a lattice of `spacing` below the points keep_out [k, 2] (the scenario
    bodies, and where they may get to): at least `clear` from each of them, and outside the strip
    that each ray (p1, p2) sweeps, taken along its whole line. Bodies of `radius` parked there
    neither touch nor share a fat AABB overlap when spacing > 2 * (radius + 0.1)."""
    keep = np.asarray(keep_out, np.float64).reshape(-1, 2)
    ends = np.asarray([q for r in rays for q in r], np.float64).reshape(-1, 2)
    pts = np.concatenate([keep, ends])
    x0 = np.ceil(pts[:, 0].max()) + 2.0 if len(rays) else np.floor(pts[:, 0].min())  # right of every upward ray
    y0 = np.floor(pts[:, 1].min() - clear - spacing)
    k = np.arange(n)
    p = np.stack([x0 + (k % cols) * spacing, y0 - (k // cols) * spacing], -1)
    if n:
        assert spacing > 2 * (radius + float(AABB_EXT))
        assert np.sqrt(((p[:, None] - keep[None]) ** 2).sum(-1)).min() >= clear
        for p1, p2 in rays:
            p1, d = np.asarray(p1, np.float64), np.asarray(p2, np.float64) - np.asarray(p1, np.float64)
            off = np.abs((p[:, 0] - p1[0]) * d[1] - (p[:, 1] - p1[1]) * d[0]) / np.hypot(*d)
            assert off.min() > 2 * radius, "a filler inside a ray's strip"
    return p.astype(np.float32)


# ---- Flock scenarios: groups of (pos [k, 2], vel [k, 2], angle [k], action [k, 3]) ---------------

def _group(pos, vel=None, angle=None, action=IDLE):
    pos = np.asarray(pos, np.float32).reshape(-1, 2)
    k = len(pos)
    vel = np.zeros((k, 2), np.float32) if vel is None else np.asarray(vel, np.float32).reshape(k, 2)
    angle = np.zeros(k, np.float32) if angle is None else np.asarray(angle, np.float32).reshape(k)
    return dict(pos=pos, vel=vel, angle=angle, action=np.tile(np.asarray(action, np.uint8), (k, 1)))


SUB_EPS_DELTAS = [F(0.0), F(2.0 ** -30), F(2.0 ** -24), step_f32(EPS, -1), EPS, step_f32(EPS, +1), F(2.0 ** -20)]


def sub_eps_pairs(extra=(), vel0=(0.0, 0.0)):
    """Scenario a (and b with extra = (0.5,)): two bodies whose centres are delta apart in x, delta
    around b2_epsilon. b2WorldManifold::Initialize keeps the normal (1, 0) when the squared distance is
    not above eps^2; the position solver's Normalize returns the vector as it is below eps. vel0: the
    velocity of the body at the group's origin (the other is at rest)."""
    return [_group([[0.0, 0.0], [d, 0.0]], vel=[vel0, (0.0, 0.0)]) for d in list(SUB_EPS_DELTAS) + [F(x) for x in extra]]


FAST_SPEEDS = [100.0, 119.0, 119.9, 120.0, 120.1, 121.0, 130.0, 300.0, 5000.0]
FAST_SPEEDS += [137.0, 211.0, 523.0, 1009.0, 2503.0]  # more clamped samples: the clamp's ratio is a quotient by a square root
FAST_DIRS = [(1.0, 0.0), (0.6, 0.8)]


def fast_bodies():
    """Scenario c: lone bodies with injected speeds around b2_maxTranslation / dt = 120 m/s at 60 Hz,
    along an axis and along (0.6, 0.8), and one touching pair (centres 0.9 apart) whose first body is
    driven into the second at 300 m/s."""
    g = [_group([[0.0, 0.0]], vel=[[F(s) * F(dx), F(s) * F(dy)]]) for s in FAST_SPEEDS for dx, dy in FAST_DIRS]
    g.append(_group([[0.0, 0.0], [0.9, 0.0]], vel=[[300.0, 0.0], [0.0, 0.0]]))
    return g


def touching_pairs(radius=0.5):
    """Scenario d: two bodies facing each other, centres 2r + k float32 places apart (k = -4 .. 4,
    b2CollideCircles' distSqr > radius^2 decision), both walking forward."""
    two_r = F(F(radius) + F(radius))
    return [_group([[0.0, 0.0], [step_f32(two_r, k), 0.0]], angle=[0.0, F(np.pi)], action=FORWARD)
            for k in range(-4, 5)]


def flock_layout(groups, N, one_per_env, alternate=True, spacing=1.5, radius=0.5, E=2):
    """pos, vel, angle [E, N, ...], first-step actions [E, N, 3] and, per env, the (group, body indices)
    placed in it. one_per_env: env e holds group e at the origin (E = len(groups)); else every env
    holds all groups, group k at (0, 10 k): offsets inside a group are in x, so they stay
    representable. Group k of env e lists its bodies in reverse index order when e + k is odd, so
    that each group meets both orders over two envs (or as two consecutive copies in one env). The
    other bodies are parked (park_fillers)."""
    per_env = [[g] for g in groups] if one_per_env else [list(groups) for _ in range(E)]
    E = len(per_env)
    pos = np.zeros((E, N, 2), np.float32)
    vel = np.zeros((E, N, 2), np.float32)
    ang = np.zeros((E, N), np.float32)
    act = np.ones((E, N, 3), np.uint8)
    where = []
    for e, gs in enumerate(per_env):
        i, placed = 0, []
        for k, g in enumerate(gs):
            n = len(g["pos"])
            idx = np.arange(i, i + n)
            if alternate and (e + k) % 2:
                idx = idx[::-1]
            pos[e, idx] = g["pos"] + np.array([0.0, 10.0 * k], np.float32)
            vel[e, idx], ang[e, idx], act[e, idx] = g["vel"], g["angle"], g["action"]
            placed.append((g, idx))
            i += n
        assert i <= N
        pos[e, i:] = park_fillers(N - i, pos[e, :i], spacing=spacing, radius=radius)
        where.append(placed)
    return pos, vel, ang, act, where


# ---- TDM ray-cast scenarios --------------------------------------------------------------------

def body(dx, dy, angle=0.0, team=1, attack=False, alive=1, health=1.0):
    return dict(d=(F(dx), F(dy)), angle=F(angle), team=team, attack=attack, alive=alive, health=health)


def attacker(dx=0.0, dy=0.0, angle=0.0, team=0):
    return body(dx, dy, angle, team=team, attack=True)


HALF_PI = F(np.pi / 2)


def raycast_groups():
    """The ray-cast scenarios: name, bodies in index order (team 0 before team 1), where the group may
    stand ('x': on the x axis, its offsets in y need y near 0; 'y': on the y axis; 'off': rays that
    do not run along +x, in a column of their own) and the expected hit of each attacker (index in
    the group, -1 a miss; absent where the float32 arithmetic decides)."""
    g = []

    def add(name, bodies, axis="y", expect=None):
        g.append(dict(name=name, bodies=bodies, axis=axis, expect=expect or {}))

    for k in range(-4, 9):  # sigma ~ -4 k ulp: around the tangent
        add(f"tangent{k:+d}", [attacker(), body(1.5, step_f32(0.5, k))], "x", {0: 1} if k == 1 else None)
    for k in (-1, 0, 1):    # the entry point at a == maxFraction * rr
        add(f"range{k:+d}", [attacker(), body(step_f32(2.5, k), 0.0)], "y", {0: 1 if k <= 0 else -1})
    for x, y in ((1.5, 0.25), (2.25, 0.125)):  # equal a: the later body wins
        add(f"tie{x}+-", [attacker(), body(x, y), body(x, -y)], "y", {0: 2})
        add(f"tie{x}-+", [attacker(), body(x, -y), body(x, y)], "y", {0: 2})
    add("behind", [attacker(), body(-1.5, 0.0)], "y", {0: -1})
    add("inside", [attacker(), body(0.25, 0.125)], "y", {0: -1})
    add("inside_then_farther", [attacker(), body(0.25, 0.125), body(1.75, 0.0)], "y", {0: 2})
    add("two_in_line", [attacker(), body(2.375, 0.0), body(1.25, 0.0)], "y", {0: 2})
    add("two_in_line_up", [attacker(angle=HALF_PI), body(0.0, 2.375), body(0.0, 1.25)], "off", {0: 2})
    add("dead_in_front", [attacker(), body(1.125, 0.0, alive=0, health=0.0), body(2.375, 0.0)], "y", {0: 2})
    add("ally_in_front", [body(2.375, 0.0, team=0), attacker(team=1), body(1.25, 0.0)], "y", {1: 2})
    # the shared listener (fresh_raycast = 0): a miss after a hit damages the last-hit body again
    add("miss_after_hit", [body(0.0, 0.0, team=0), attacker(-1.5, 0.0, team=1),
                           attacker(0.0, -3.0, angle=-HALF_PI, team=1)], "off", {1: 0, 2: -1})
    # three hits on health 0.5: the third lands on a body already at 0, still alive within the step
    add("three_on_one", [body(0.0, 0.0, team=0, health=0.5), attacker(-1.5, 0.0, team=1),
                         attacker(1.5, 0.0, angle=F(np.pi), team=1), attacker(0.0, -1.5, angle=HALF_PI, team=1)],
        "off", {1: 0, 2: 0, 3: 0})
    return g


def tdm_layout(per_env, teams):
    """Arrays [E, N, ...] for inject_tdm and the first step from per_env, one list of groups per env:
    pos, angle, alive, health, attack (bool), and per env the (group, agent indices) placed. Each
    team's indices are handed out in group order, the rest are fillers (alive, idle, parked). A single
    group stands at the origin; several stand at multiples of 16 m on their axis."""
    from raycast_ref import ray_end
    E, N = len(per_env), sum(teams)
    first = np.concatenate([[0], np.cumsum(teams)])
    pos = np.zeros((E, N, 2), np.float32)
    ang = np.zeros((E, N), np.float32)
    alive = np.ones((E, N), np.uint8)
    health = np.ones((E, N), np.float64)
    attack = np.zeros((E, N), bool)
    where = []
    for e, gs in enumerate(per_env):
        nxt = [int(first[t]) for t in range(len(teams))]
        count = dict(x=0, y=0, off=0)
        used, rays, placed = [], [], []
        for g in gs:
            k = count[g["axis"]]
            count[g["axis"]] += 1
            if len(gs) == 1:
                org = (0.0, 0.0)
            else:
                org = {"x": (16.0 * k, 0.0), "y": (0.0, 16.0 * (k + 1)), "off": (-48.0 - 16.0 * k, 8.0 + 16.0 * k)}[g["axis"]]
            idx = []
            for b in g["bodies"]:
                i = nxt[b["team"]]
                nxt[b["team"]] += 1
                assert i < first[b["team"] + 1], "a team has too few agents for these groups"
                assert not idx or i > idx[-1], "index order within a group follows the list"
                idx.append(i)
                pos[e, i] = (F(org[0]) + b["d"][0], F(org[1]) + b["d"][1])
                assert pos[e, i, 0] - F(org[0]) == b["d"][0] and pos[e, i, 1] - F(org[1]) == b["d"][1], "offset lost"
                ang[e, i], alive[e, i], health[e, i], attack[e, i] = b["angle"], b["alive"], b["health"], b["attack"]
                if b["attack"]:
                    rays.append((pos[e, i], ray_end(pos[e, i], b["angle"])))
            used += idx
            placed.append((g, np.array(idx)))
        free = np.setdiff1d(np.arange(N), used)
        pos[e, free] = park_fillers(len(free), pos[e, used], rays)
        where.append(placed)
    return pos, ang, alive, health, attack, where


def attack_actions(attack):
    """[E, N, 4]: the attack action alone for the attackers (no move, no turn: the cast happens
    before the physics), idle for the rest."""
    a = np.ones(attack.shape + (4,), np.uint8)
    a[..., 3] = attack
    return a


def split_groups(groups, n_envs):
    """groups dealt to n_envs envs in contiguous runs of about equal body count."""
    total = sum(len(g["bodies"]) for g in groups)
    out, cur, acc = [], [], 0
    for g in groups:
        if cur and len(out) < n_envs - 1 and acc + len(g["bodies"]) > total * (len(out) + 1) / n_envs:
            out.append(cur)
            cur = []
        cur.append(g)
        acc += len(g["bodies"])
    out.append(cur)
    return out


def expected_health(pos, ang, alive, health, attack, fresh, dmg=0.25, radius=0.5):
    """The health [E, N] after the attackers' casts, from raycast_ref.raycast_f32 on the injected
    poses and the reference's listener (combat.py:121-155, cm_framework.py:56-86): in agent order,
    a hit damages its body; with the shared listener (fresh = 0, nothing hit before) a miss damages
    the body hit last, once anything has been hit. Also the hit index of every attacker."""
    from raycast_ref import ray_end, raycast_f32
    hp = np.array(health, np.float64)
    hits = np.full(pos.shape[:2], -2, np.int32)
    for e in range(pos.shape[0]):
        last = -1
        for i in np.nonzero(attack[e] & (alive[e] != 0))[0]:
            h, _ = raycast_f32(pos[e], radius, pos[e, i], ray_end(pos[e, i], ang[e, i]), alive[e])
            hits[e, i] = h
            if fresh:
                if h >= 0:
                    hp[e, h] -= dmg
            else:
                if h >= 0:
                    last = h
                if last >= 0:
                    hp[e, last] -= dmg
    return hp, hits


TDM_FORMS = {  # teams, envs the groups are dealt to (None: one group per env), world side
    "wave32": ([1, 3], None, 30.0),
    "wave64": ([32, 32], 2, 200.0),
    "workgroup": ([33, 32], 2, 200.0),
    "two_per_thread": ([513, 512], 1, 200.0),
}


def tdm_form(name):
    """(teams, world keywords, tdm_layout's arrays) of one form of the ray-cast scenarios."""
    teams, n_envs, side = TDM_FORMS[name]
    groups = raycast_groups()
    per_env = [[g] for g in groups] if n_envs is None else split_groups(groups, n_envs)
    return teams, dict(world_width=side, world_height=side), tdm_layout(per_env, teams)


def flock_scenario(name):
    """Scenarios a-d of the Flock step (and a with one body of each pair moving into the other, where
    the fallback normal shows in the velocities): the groups, the settings keywords beyond the defaults, the
    body radius and filler spacing, the number of steps that repeat the layout's first actions
    (`hold`) and the random steps after them."""
    from gym_macm.settings import CircleFixture
    big = dict(fixtures=CircleFixture(0.8, 1.0, 0.3), linearDamping=5, fixedRotation=True)
    undamped = dict(fixtures=CircleFixture(0.5, 1.0, 0.3), linearDamping=0, fixedRotation=True)
    s = {
        "sub_eps": dict(groups=sub_eps_pairs(), hold=2, random=3),
        "sub_eps_r08": dict(groups=sub_eps_pairs(extra=(0.5,)), kw=dict(bodySettings=big), radius=0.8, spacing=2.4,
                            hold=2, random=3),
        # every pair twice: one_per_env then puts each delta into an even and an odd (reversed) env
        "sub_eps_moving": dict(groups=[g for g in sub_eps_pairs(vel0=(1.0, 0.0)) for _ in range(2)], hold=2, random=2),
        "fast": dict(groups=fast_bodies(), kw=dict(hz=60.0), hold=2, random=0),
        "fast_undamped": dict(groups=fast_bodies(), kw=dict(hz=60.0, bodySettings=undamped), hold=2, random=0),
        "touching": dict(groups=touching_pairs(), hold=3, random=0),
    }[name]
    return dict(dict(kw={}, radius=0.5, spacing=1.5), name=name, **s)


FLOCK_SCENARIOS = ("sub_eps", "sub_eps_r08", "sub_eps_moving", "fast", "fast_undamped", "touching")


def scenario_actions(sc, act, rng):
    """actions_fn(t) of a scenario: the layout's actions for `hold` steps, then random ones."""
    def fn(t):
        return act if t < sc["hold"] else rng.integers(0, 3, size=act.shape).astype(np.uint8)
    return fn
