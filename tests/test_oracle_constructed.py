"""The constructed scenarios of tests/constructed.py on the CPU oracle alone, without a GPU: each one
must reach the branch it was built for, shown from observable outputs, so that the device tests
(test_gpu_constructed_flock.py, test_gpu_tdm_raycast.py) cannot pass without comparing that branch.
Both sides of every boundary must appear, and everything stays finite."""
import numpy as np
import pytest

import constructed as cs
from oracle import OracleFlock, OracleTDM
from gym_macm.settings import flockSettings, to_config
from gym_macm.tdm_world import tdm_config

F = np.float32


def flock_oracle(sc, N, one_per_env, seed=1):
    pos, vel, ang, act, where = cs.flock_layout(sc["groups"], N, one_per_env, spacing=sc["spacing"], radius=sc["radius"])
    E = pos.shape[0]
    kw = dict(start_spread=200, **sc["kw"])
    orc = OracleFlock(to_config(flockSettings(**kw), N, 1, obs_f64=True), None, E, seed)
    cs.inject(None, orc, pos, vel=vel, angle=ang, radius=sc["radius"], capacity=64)
    return orc, pos, vel, act, where


def centre_distance(st, e, idx):
    d = st["pos"][e, idx[1]].astype(np.float64) - st["pos"][e, idx[0]].astype(np.float64)
    return float(np.hypot(*d))


def all_finite(orc, r):
    st = orc.get_state(64)
    return all(np.isfinite(st[k]).all() for k in ("pos", "vel", "angle", "fat")) and np.isfinite(r["obs"]).all()


@pytest.mark.parametrize("name,N,one_per_env", [("sub_eps", 4, True), ("sub_eps", 64, False),
                                                 ("sub_eps_r08", 4, True), ("sub_eps_r08", 65, False)])
def test_sub_eps_pairs_take_the_fallback_normal(name, N, one_per_env):
    """Two no-op steps on pairs whose centres start delta apart, then three random steps.

    While the distance d is below eps, the position solver's Normalize returns (d, 0) as it is, the
    separation is d * d - 2r, and one iteration moves the pair apart by 0.2 * (2r - slop) * d: d
    grows by the factor 1.199 (1.2 at r = 0.8, the clamp) per iteration, three iterations a step. From
    eps on the normal is a unit vector and one iteration adds min(0.2, 0.2 * (2r - slop - d)).
      delta = 0         exactly coincident after both steps (and each the other's neighbour at r = 0)
      delta = 2^-30     below 1e-6 after both steps (1.2^6 * 2^-30; measured 2.8e-9)
      delta = 2^-24     below 1e-6 after the first step (1.72 * 2^-24 < eps), crosses eps in the second
                        and ends more than 0.1 apart (measured 0.358)
      delta = eps-      one iteration below eps, then two pushes: after the first step more than 0.1
                        apart and more than 0.1 short of delta = eps (measured 0.358 and 0.486)
      delta >= eps      three pushes in the first step; more than 0.1 apart (measured 0.486, then 0.734)
    With radius 0.8 the separation is below -1.005, so every push of the first step is the clamped
    0.2 exactly: 0.6 after one step from eps on, 0.4 from eps- (within 1e-5)."""
    sc = cs.flock_scenario(name)
    r08 = sc["radius"] == 0.8
    if r08:
        for g in sc["groups"]:
            assert float(g["pos"][1, 0]) - 1.6 < -1.005
    orc, pos, vel, act, where = flock_oracle(sc, N, one_per_env)
    states = []
    for _ in range(2):
        r = orc.step(act)
        states.append(orc.get_state(64))
    assert all_finite(orc, r)
    eps, below = float(cs.EPS), float(cs.step_f32(cs.EPS, -1))
    seen = set()
    for e, placed in enumerate(where):
        d1, d2 = {}, {}
        for g, idx in placed:
            delta = float(g["pos"][1, 0])
            d1[delta], d2[delta] = (centre_distance(st, e, idx) for st in states)
            seen.add(delta)
            if delta == 0.0:
                for st in states:
                    np.testing.assert_array_equal(st["pos"][e, idx[0]], st["pos"][e, idx[1]])
                # each is the other's nearest neighbour, at distance 0: atan2(0, 0) in the observation
                assert r["nbr_id"][e, idx[0]] == idx[1] and r["obs"][e, idx[0], 0] == 0.0
            elif delta == 2.0 ** -30:
                assert d1[delta] - delta < 1e-6 and d2[delta] - delta < 1e-6 and d2[delta] > d1[delta] > delta
            elif delta == 2.0 ** -24:
                assert delta < d1[delta] < eps and d2[delta] - delta > 0.1
            else:
                assert d1[delta] - delta > 0.1 and d2[delta] - delta > 0.1, (delta, d1[delta], d2[delta])
            if r08 and eps <= delta < 0.1:
                assert abs(d1[delta] - delta - 0.6) < 1e-5, (delta, d1[delta])
        if not one_per_env:
            assert d1[eps] - d1[below] > 0.1 and d1[eps] == d1[float(cs.step_f32(cs.EPS, 1))]
            if r08:
                assert abs(d1[below] - 0.4) < 1e-5
    assert seen >= {float(d) for d in cs.SUB_EPS_DELTAS}
    rng = np.random.default_rng(0)
    for _ in range(3):
        r = orc.step(rng.integers(0, 3, size=act.shape).astype(np.uint8))
    assert all_finite(orc, r)


@pytest.mark.parametrize("N,one_per_env", [(4, True), (64, False)])
def test_fallback_normal_shows_in_the_velocities(N, one_per_env):
    """One body of each pair moves at 1 m/s along +x into the other. In reversed index order fixture
    B is the moving body on the -x side of A: the geometric normal is (-1, 0) and the contact shares
    the momentum, but at or below eps the normal stays (1, 0), the relative normal velocity is
    positive, no impulse acts and the body at rest keeps velocity 0 exactly. In forward order both
    normals are (1, 0) and every pair shares the momentum."""
    sc = cs.flock_scenario("sub_eps_moving")
    orc, pos, vel, act, where = flock_oracle(sc, N, one_per_env)
    orc.step(act)
    st = orc.get_state(64)
    seen = set()
    for e, placed in enumerate(where):
        for g, idx in placed:
            delta, at_rest = float(g["pos"][1, 0]), st["vel"][e, idx[1]]
            reverse = idx[0] > idx[1]
            if reverse and delta <= float(cs.EPS):
                assert at_rest[0] == 0.0 and at_rest[1] == 0.0, (delta, at_rest)
            else:
                assert at_rest[0] > 0.1, (delta, reverse, at_rest)
            seen.add((delta, bool(reverse)))
    assert seen == {(float(d), o) for d in cs.SUB_EPS_DELTAS for o in (False, True)}


@pytest.mark.parametrize("name", ["fast", "fast_undamped"])
@pytest.mark.parametrize("N,one_per_env", [(4, True), (64, False)])
def test_fast_bodies_reach_the_translation_clamp(name, N, one_per_env):
    """At least 4 bodies whose injected dt * |v| exceeds b2_maxTranslation = 2 move 2 m (within 1e-5)
    in the first step, at least 3 move less; without damping the boundary speed 120 m/s is among the
    bodies stepped."""
    sc = cs.flock_scenario(name)
    orc, pos, vel, act, where = flock_oracle(sc, N, one_per_env)
    assert np.isfinite(vel).all() and np.abs(vel).max() <= 5000.0
    r = orc.step(act)
    st = orc.get_state(64)
    moved = np.hypot(*np.moveaxis(st["pos"].astype(np.float64) - pos.astype(np.float64), -1, 0))
    over = np.hypot(*np.moveaxis(vel.astype(np.float64), -1, 0)) / 60.0 > 2.0
    lone = np.zeros(moved.shape, bool)
    for e, placed in enumerate(where):
        for g, idx in placed:
            if len(idx) == 1:
                lone[e, idx] = True
    per_env = 1 if one_per_env else pos.shape[0]
    assert (lone & over & (np.abs(moved - 2.0) < 1e-5)).sum() >= 4 * per_env
    assert (lone & (vel != 0).any(-1) & (moved < 2.0 - 1e-5)).sum() >= 3 * per_env
    assert (moved[lone] <= 2.0 + 1e-5).all(), "no lone body moves farther than b2_maxTranslation"
    r = orc.step(act)
    assert all_finite(orc, r)


def test_touching_decision_has_both_sides():
    """Centres 2r + k places apart: k <= 0 touches at once and is held (closing under 1e-3 in the
    first step), k > 0 closes freely for one step (the two bodies' forward push, over 5e-3)."""
    sc = cs.flock_scenario("touching")
    orc, pos, vel, act, where = flock_oracle(sc, 64, False)
    r = orc.step(act)
    st = orc.get_state(64)
    held = free = 0
    for e, placed in enumerate(where):
        for (g, idx), k in zip(placed, range(-4, 5)):
            closing = float(g["pos"][1, 0]) - centre_distance(st, e, idx)
            if k <= 0:
                assert abs(closing) < 1e-3, (k, closing)
                held += 1
            else:
                assert closing > 5e-3, (k, closing)
                free += 1
    assert held and free
    for _ in range(2):
        r = orc.step(act)
    assert all_finite(orc, r)


# ---- TDM: the ray-cast scenarios ------------------------------------------------------------------

def tdm_oracle(form, fresh):
    teams, kw, (pos, ang, alive, health, attack, where) = cs.tdm_form(form)
    orc = OracleTDM(tdm_config(teams, obs_f64=True, fresh_raycast=fresh, **kw), pos.shape[0], 3)
    cs.inject_tdm(None, orc, pos, ang, alive, health)
    return orc, pos, ang, alive, health, attack, where


@pytest.mark.parametrize("fresh", [1, 0])
@pytest.mark.parametrize("form", list(cs.TDM_FORMS))
def test_raycast_scenarios_on_the_oracle(form, fresh):
    """Every attacker hits what the scenario says (per group where the casts do not share a
    listener), and the oracle's health equals the numpy restatement's for the whole env."""
    orc, pos, ang, alive, health, attack, where = tdm_oracle(form, fresh)
    r = orc.step(cs.attack_actions(attack))
    want, hits = cs.expected_health(pos, ang, alive, health, attack, fresh)
    np.testing.assert_array_equal(r["health"], want)
    assert np.isfinite(r["obs"]).all() and np.isfinite(orc.get_state()["pos"]).all()
    tangent = {}
    for e, placed in enumerate(where):
        for g, idx in placed:
            for a, h in g["expect"].items():
                assert hits[e, idx[a]] == (idx[h] if h >= 0 else -1), (g["name"], a)
            if g["name"].startswith("tangent"):
                tangent[int(g["name"][7:])] = int(hits[e, idx[0]])
            if fresh or len(placed) == 1:  # this group's casts alone decide its bodies' health
                dmg = {int(i): 0.0 for i in idx}
                last = -1
                for a in np.nonzero(attack[e, idx])[0]:
                    h = int(hits[e, idx[a]])
                    last = h if h >= 0 else last
                    tgt = h if fresh else last
                    if tgt >= 0:
                        dmg[tgt] += 0.25
                for i in idx:
                    assert r["health"][e, i] == health[e, i] - dmg[int(i)], (g["name"], int(i))
            if g["name"] == "three_on_one":
                assert r["health"][e, idx[0]] == -0.25 and r["alive"][e, idx[0]] == 0
            if g["name"] == "miss_after_hit" and len(placed) == 1:
                assert r["health"][e, idx[0]] == (0.75 if fresh else 0.5)
            if g["name"] == "dead_in_front":
                assert r["health"][e, idx[1]] == 0.0 and r["alive"][e, idx[1]] == 0
    assert sorted(tangent) == list(range(-4, 9)) and tangent[1] >= 0
    assert {h >= 0 for h in tangent.values()} == {True, False}, "the tangent sweep holds both outcomes"
