"""Reset poses drawn from Python's own ``random`` (tests/ only): what include/macm.h promises for
macm_world_reset / macm_tdm_reset (env e is the reference env after ``random.seed(seed + env_offset + e)``)
and for the reset_envs calls (each env continues that stream), stated with CPython's generator itself
instead of the project's two restatements of it (csrc/py_mt19937.hpp, oracle/pyrandom.c). The draw
order is the reference's (mvmnt.py:47-64 and :224-233, combat.py:80-95 and :234-245), as the drop-in
envs (gym_macm/envs) draw it from the global ``random``."""
import math
import random

import numpy as np

# (seed, env_offset): one-word keys next to two-word keys inside one batch (2**32 - 2, 2**32 - 1, 2**32, ...),
# a two-word key, the top bit of the second word reached inside the batch, a key that is two words only
# through env_offset, and the last seeds below 2**64
SEED_PAIRS = [((1 << 32) - 2, 0), ((1 << 32) + 7, 0), ((1 << 63) - 3, 1), (5, (1 << 32) - 3), ((1 << 64) - 4, 0)]


def streams(E, seed, env_offset):
    """One generator per env, seeded as random.seed(seed + env_offset + e) seeds the global one."""
    return [random.Random(seed + env_offset + e) for e in range(E)]


def flock_targets(r, cfg):
    tg = np.zeros((cfg.n_targets, 2), np.float32)
    for t in range(cfg.n_targets):
        rand_angle = 2 * math.pi * r.random()
        rand_dist = cfg.target_mindist + r.random() * (cfg.target_maxdist - cfg.target_mindist)
        tg[t] = (rand_dist * math.cos(rand_angle), rand_dist * math.sin(rand_angle))
    return tg


def flock_agents(r, cfg):
    N = cfg.n_agents
    pos, ang = np.zeros((N, 2), np.float32), np.zeros((N,), np.float32)
    for i in range(N):
        x = cfg.start_spread * (r.random() - 0.5) + cfg.start_point[0]
        y = cfg.start_spread * (r.random() - 0.5) + cfg.start_point[1]
        ang[i] = r.uniform(-1, 1) * math.pi
        pos[i] = (x, y)
    return pos, ang


def tdm_agents(r, cfg):
    N = cfg.n_agents
    pos, ang = np.zeros((N, 2), np.float32), np.zeros((N,), np.float32)
    k = 0
    for team in range(cfg.n_teams):
        for _ in range(cfg.team_size[team]):
            x = r.random() * (team + cfg.world_width / 2)
            y = r.random() * cfg.world_height
            ang[k] = r.uniform(-1, 1) * math.pi
            pos[k] = (x, y)
            k += 1
    return pos, ang


def flock_reset(rs, cfg):
    """Flock.__init__'s draws of every env's stream: (pos [E, N, 2], angle [E, N], targets [E, T, 2])."""
    tg = [flock_targets(r, cfg) for r in rs]
    pa = [flock_agents(r, cfg) for r in rs]
    return np.stack([p for p, _ in pa]), np.stack([a for _, a in pa]), np.stack(tg)


def tdm_reset(rs, cfg):
    pa = [tdm_agents(r, cfg) for r in rs]
    return np.stack([p for p, _ in pa]), np.stack([a for _, a in pa])


def redraw(rs, cfg, mask, pos, ang, agents):
    """reset_envs: the masked envs draw their next agent poses (agents: flock_agents or tdm_agents) into
    pos / angle in place; the others keep theirs and their streams do not advance."""
    for e, r in enumerate(rs):
        if mask[e]:
            pos[e], ang[e] = agents(r, cfg)
