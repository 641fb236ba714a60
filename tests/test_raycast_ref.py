"""tests/raycast_ref.py against the oracle's b2l_world_raycast (oracle.B2World.raycast), without a
GPU: the numpy float32 restatement gives the same hit index and bitwise the same fraction, on random
rays and on every boundary scenario of tests/constructed.raycast_groups; where the float64 geometry
decides with a margin, the float32 hit is the geometric one. The device tests
(test_gpu_tdm_raycast.py) then have a third, independent opinion on every hit."""
import numpy as np
import pytest

from constructed import raycast_groups
from oracle import B2World
from raycast_ref import ray_end, raycast_f32, raycast_f64

MARGIN = 1e-4


def world_of(centres, radius, active=None):
    w = B2World()
    for i, (x, y) in enumerate(centres):
        w.create_body(float(x), float(y), 0.0, radius, 1.0, 0.3, 5.0, True)
    for i in range(len(centres)):
        if active is not None and not active[i]:
            w.set_active(i, 0)
    return w


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def test_random_rays_bitwise_equal_and_geometrically_right():
    rng = np.random.default_rng(2024)
    rays = decided = hits = 0
    for n in range(2, 13):
        radius = float(rng.choice([0.5, 0.8, 0.3]))
        w = world_of(np.zeros((n, 2)), radius)
        for _ in range(300):
            c = rng.uniform(-2, 2, size=(n, 2)).astype(np.float32)
            for i in range(n):
                w.set_transform(i, float(c[i, 0]), float(c[i, 1]), 0.0)
            # a third of the rays start at a body's centre, as an attacker's does
            p1 = c[rng.integers(n)] if rng.random() < 1 / 3 else rng.uniform(-2, 2, size=2).astype(np.float32)
            p2 = ray_end(p1, rng.uniform(-np.pi, np.pi), reach=float(rng.choice([2.0, 0.5, 4.0])))
            hit_o, fr_o = w.raycast(float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1]))
            hit_r, fr_r = raycast_f32(c, radius, p1, p2)
            assert hit_r == hit_o and same_bits(fr_r, fr_o), (n, c, p1, p2, hit_o, fr_o, hit_r, fr_r)
            hit_d, fr_d, mfrac, mlat = raycast_f64(c, radius, p1, p2)
            rays += 1
            if mfrac >= MARGIN and mlat >= MARGIN:
                decided += 1
                hits += hit_d >= 0
                assert hit_r == hit_d, (c, p1, p2, hit_r, hit_d, mfrac, mlat)
                assert abs(float(fr_r) - fr_d) < 1e-5
    assert rays >= 3000 and decided > 0.9 * rays and hits > 0.2 * rays, (rays, decided, hits)


@pytest.mark.parametrize("group", raycast_groups(), ids=lambda g: g["name"])
def test_boundary_scenarios_bitwise_equal(group):
    bodies = group["bodies"]
    c = np.array([b["d"] for b in bodies], np.float32)
    active = [b["alive"] for b in bodies]
    w = world_of(c, 0.5, active)
    for i, b in enumerate(bodies):
        if not b["attack"]:
            continue
        p2 = ray_end(c[i], b["angle"])
        hit_o, fr_o = w.raycast(float(c[i, 0]), float(c[i, 1]), float(p2[0]), float(p2[1]))
        hit_r, fr_r = raycast_f32(c, 0.5, c[i], p2, active)
        assert hit_r == hit_o and same_bits(fr_r, fr_o), (group["name"], hit_o, fr_o, hit_r, fr_r)
        if i in group["expect"]:
            assert hit_o == group["expect"][i], group["name"]
        hit_d, _, mfrac, mlat = raycast_f64(c, 0.5, c[i], p2, active)
        if mfrac >= MARGIN and mlat >= MARGIN:
            assert hit_r == hit_d, group["name"]


def test_tangent_sweep_holds_both_outcomes():
    """The sweep over (1.5, 0.5 + k places) crosses from hit to miss, and float64 agrees that the
    circle at k = 0 touches the ray's line (margin 0), so only float32 rounding decides there."""
    out = {}
    for g in raycast_groups():
        if g["name"].startswith("tangent"):
            c = np.array([b["d"] for b in g["bodies"]], np.float32)
            out[int(g["name"][7:])] = raycast_f32(c, 0.5, c[0], ray_end(c[0], 0.0))[0]
    assert sorted(out) == list(range(-4, 9))
    assert out[-4] == 1 and out[1] == 1 and out[8] == -1
    ks = sorted(out)
    assert all(out[a] >= out[b] for a, b in zip(ks, ks[1:])), "one crossing from hit to miss"
    c0 = np.array([[0.0, 0.0], [1.5, 0.5]])
    assert raycast_f64(c0, 0.5, c0[0], (2.0, 0.0))[3] == 0.0
