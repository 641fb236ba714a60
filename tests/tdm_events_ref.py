"""Reference for the TDM combat events (macm_tdm_set_events), tests/ only.

The oracle (oracle/tdm_oracle.c) steps TDM as the reference does and does not report victims, so
they are derived from it: `derive_events` takes the oracle's state before a step and the step's
actions and replays the action loop's melee part (combat.py:121-155) in agent order,
  attackers = alive & cooldown_atk <= 0 & attack bit,
  the rotated float32 angle as the step computes it, float32(float64(angle) + (a2 - 1) *
  rotation_speed * (1 / hz)), then the +-2 pi wrap,
  p2 = p1 + float32(range * cos, range * sin) (math.cos / math.sin),
  the cast: raycast_ref.raycast_f32 over the start-of-step positions of the bodies alive at the
  step's start (bodies neither move nor die inside the action loop),
  the listener rule, literal (shared, never reset) or fresh_raycast,
and returns hit_id, the replayed health and the listener. That the replay is the oracle's is what
test_tdm_events_ref.py checks: health and listener after every step of every fixture, bit for bit.

An exact float32 prefilter drops the candidates no cast can accept (sigma < 0, a < 0, a > rr: the
clip fraction never exceeds 1, and float32 multiplication by a value <= 1 is monotone), which keeps
the 2100-agent fixture short; the accepted order among the rest is raycast_f32's.

`FIXTURES` are the worlds the events tests run, `run_fixture` the oracle trajectory of one (cached:
the GPU tests and the CPU tests share it and must not modify it).
"""
import functools
import math

import numpy as np
from raycast_ref import EPS, F, raycast_f32

from gym_macm.tdm_world import tdm_config
from oracle import OracleTDM


def rotated_angle(angle, a2, rotation_speed, hz):
    """The body's float32 angle after the step's SetTransform (combat.py:128-133)."""
    af = F(float(angle) + (float(int(a2) - 1) * float(rotation_speed)) * (1.0 / float(hz)))
    ad = float(af)
    if abs(ad) > math.pi:
        af = F(ad - math.copysign(1.0, ad) * (2.0 * math.pi))
    return af


def _candidates(centres, idx, radius, p1, p2):
    """The bodies of `idx` a cast from p1 to p2 could accept at all, in body order (exact float32)."""
    c = centres[idx]
    x1, y1, x2, y2 = F(p1[0]), F(p1[1]), F(p2[0]), F(p2[1])
    rad = F(radius)
    sx, sy = x1 - c[:, 0], y1 - c[:, 1]
    b = (sx * sx + sy * sy) - F(rad * rad)
    rx, ry = F(x2 - x1), F(y2 - y1)
    cc = sx * rx + sy * ry
    rr = F(F(rx * rx) + F(ry * ry))
    sigma = cc * cc - rr * b
    if rr < EPS:
        return idx[:0]
    with np.errstate(invalid="ignore"):
        a = -(cc + np.sqrt(sigma))
    assert sx.dtype == np.float32 and a.dtype == np.float32
    return idx[(sigma >= F(0.0)) & (a >= F(0.0)) & (a <= rr)]


def derive_events(cfg, state, actions, with_rays=False):
    """(hit_id [E, N] int32, health [E, N] float64, listener [E, 2] int32) of one step from the
    oracle's pre-step `state` (OracleTDM.get_state()) and `actions` [E, N, 4] uint8. with_rays: also
    the body each attacker's own ray hit, or -1 ([E, N] int32)."""
    pos = np.asarray(state["pos"], np.float32)
    E, N = pos.shape[:2]
    health = np.array(state["health"], np.float64)
    lis = np.array(state["listener"], np.int32)
    hit_id = np.full((E, N), -1, np.int32)
    rays = np.full((E, N), -1, np.int32)
    dmg, reach = float(cfg.melee_dmg), float(cfg.melee_range)
    for e in range(E):
        alive = state["alive"][e] != 0
        live = np.flatnonzero(alive)
        att = alive & (state["cd_atk"][e] <= 0.0) & (actions[e, :, 3] != 0)
        for i in np.flatnonzero(att):
            af = float(rotated_angle(state["angle"][e, i], actions[e, i, 2], cfg.agent_rotation_speed, cfg.hz))
            p1 = pos[e, i]
            p2 = (F(p1[0] + F(reach * math.cos(af))), F(p1[1] + F(reach * math.sin(af))))
            cand = _candidates(pos[e], live, cfg.radius, p1, p2)
            k, _ = raycast_f32(pos[e][cand], cfg.radius, p1, p2)
            h = int(cand[k]) if k >= 0 else -1
            rays[e, i] = h
            if cfg.fresh_raycast:
                if h >= 0:
                    health[e, h] -= dmg
                hit_id[e, i] = h
            else:
                if h >= 0:
                    lis[e] = (1, h)
                if lis[e, 0]:
                    health[e, lis[e, 1]] -= dmg
                    hit_id[e, i] = lis[e, 1]
    # (fresh_raycast: the listener is a new object per cast, the state's stays what it was)
    return (hit_id, health, lis, rays) if with_rays else (hit_id, health, lis)


# name -> (teams, E, K, seed, config overrides, reset_envs(done) after each step)
FIXTURES = {
    "W1": ((16, 16), 8, 40, 3, {}, False),
    "W2": ((16, 16), 8, 40, 3, dict(fresh_raycast=True), False),
    "W3": ((3, 3), 16, 60, 5, {}, False),
    "W4": ((32, 32), 4, 30, 7, {}, False),
    "W5": ((3, 2, 2), 16, 60, 11, dict(world_width=6.0, world_height=6.0), True),
    "W6": ((3, 2, 2), 16, 40, 11, dict(world_width=6.0, world_height=6.0, time_limit=0.2), True),
    "G1": ((40, 40), 2, 12, 13, {}, False),
    "G1f": ((40, 40), 2, 12, 13, dict(fresh_raycast=True), False),
    "G2": ((600, 500), 1, 2, 17, {}, False),
    "G3": ((1100, 1000), 1, 2, 19, dict(fresh_raycast=True), False),
}


def fixture_config(name, obs_f64=False, **more):
    teams, _, _, _, over, _ = FIXTURES[name]
    return tdm_config(teams, obs_f64=obs_f64, **{"cooldown_atk": 0.05, **over, **more})


def fixture_actions(name):
    """[K, E, N, 4] uint8: per step three integers(0, 3, (E, N)) and then integers(0, 2, (E, N))."""
    teams, E, K, seed, _, _ = FIXTURES[name]
    N = sum(teams)
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(K):
        cols = [rng.integers(0, 3, (E, N)) for _ in range(3)] + [rng.integers(0, 2, (E, N))]
        rows.append(np.stack(cols, axis=-1).astype(np.uint8))
    return np.stack(rows)


def replay(cfg, E, seed, actions, reset):
    """The oracle through `actions` [K, E, N, 4] (with `reset`: reset_envs(done) after each step) and
    the events derived from it. Per-step rows: hit_id, ray_hit (own rays), health_ref / listener_ref (the replay's),
    health / alive / done / winner / listener (the oracle's after the step), alive_before,
    health_before, cd_atk_before, listener_before, done_before; and the oracle's final state."""
    orc = OracleTDM(cfg, E, seed)
    rows = {k: [] for k in ("hit_id", "ray_hit", "health_ref", "listener_ref", "health", "alive", "done", "winner", "listener",
                            "alive_before", "health_before", "cd_atk_before", "listener_before", "done_before")}
    for a in actions:
        st = orc.get_state()
        hit, hp, lis, rays = derive_events(cfg, st, a, with_rays=True)
        r = orc.step(a)
        rows["hit_id"].append(hit)
        rows["ray_hit"].append(rays)
        rows["health_ref"].append(hp)
        rows["listener_ref"].append(lis)
        for k in ("health", "alive", "done", "winner"):
            rows[k].append(r[k].copy())
        rows["listener"].append(orc.extras()["listener"].copy())
        rows["alive_before"].append(st["alive"].copy())
        rows["health_before"].append(st["health"].copy())
        rows["cd_atk_before"].append(st["cd_atk"].copy())
        rows["listener_before"].append(st["listener"].copy())
        rows["done_before"].append(st["done"].copy())
        if reset and r["done"].any():
            orc.reset_envs(r["done"])
    out = {k: np.stack(v) for k, v in rows.items()}
    out["final_state"] = orc.get_state()
    out["actions"] = np.asarray(actions)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def run_fixture(name):
    """replay() of a fixture (computed once per process; read-only arrays)."""
    teams, E, K, seed, _, reset = FIXTURES[name]
    return replay(fixture_config(name, obs_f64=True), E, seed, fixture_actions(name), reset)


def event_counts(cfg, t):
    """Counts over a replay: attacks, damaging, stale (the damaged body is not the one the attacker's
    own ray hit), self, on bodies dead at the step's start, ally."""
    team = []
    for k in range(cfg.n_teams):
        team += [k] * cfg.team_size[k]
    team = np.array(team)
    hit = t["hit_id"]
    att = (t["alive_before"] != 0) & (t["cd_atk_before"] <= 0.0) & (t["actions"][..., 3] != 0)
    dam = hit >= 0
    assert not (dam & ~att).any()
    v = np.where(dam, hit, 0)
    idx = np.arange(hit.shape[-1])
    dead = np.take_along_axis(t["alive_before"], v, axis=-1) == 0
    return dict(attacks=int(att.sum()), damaging=int(dam.sum()), stale=int((dam & (hit != t["ray_hit"])).sum()), self=int((dam & (v == idx)).sum()),
                dead=int((dam & dead).sum()), ally=int((dam & (team[v] == team[idx])).sum()))
