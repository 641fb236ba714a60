"""Two references for the melee ray cast (tests/ only), both independent of oracle/b2lite.c.

`raycast_f32` restates b2World::RayCast with the reference's closest-hit callback
(cm_framework.py:56-86: ReportFixture keeps the fixture and returns its fraction, which clips the
rest of the cast) over circle fixtures, each tested as Box2D's b2CircleShape::RayCast tests them,
in numpy float32 with every operation rounded on its own. Candidates run in body order.

`raycast_f64` is the geometry itself in float64: the nearest circle whose entry point lies on the
segment and whose centre is more than r from the origin, with the margins of that decision, so
that a caller knows where float32 rounding cannot change the outcome.
"""
import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)  # b2_epsilon


def ray_end(p1, angle, reach=2.0):
    """point2 of the reference's melee cast (combat.py:147-149): point1 + the float32-converted tuple
    (range * cos(angle), range * sin(angle)), the angle being the body's float32 angle."""
    a = float(F(angle))
    return F(F(p1[0]) + F(reach * np.cos(a))), F(F(p1[1]) + F(reach * np.sin(a)))


def raycast_f32(centres, radius, p1, p2, active=None):
    """(index of the closest hit or -1, float32 fraction the cast ended with)."""
    x1, y1, x2, y2 = F(p1[0]), F(p1[1]), F(p2[0]), F(p2[1])
    rad = F(radius)
    max_fraction, best = F(1.0), -1
    for i, (cx, cy) in enumerate(np.asarray(centres, np.float32)):
        if active is not None and not active[i]:
            continue
        sx, sy = F(x1 - cx), F(y1 - cy)                      # s = input.p1 - position
        b = F(F(F(sx * sx) + F(sy * sy)) - F(rad * rad))     # b2Dot(s, s) - m_radius^2
        rx, ry = F(x2 - x1), F(y2 - y1)                      # r = input.p2 - input.p1
        c = F(F(sx * rx) + F(sy * ry))
        rr = F(F(rx * rx) + F(ry * ry))
        sigma = F(F(c * c) - F(rr * b))
        if sigma < F(0.0) or rr < EPS:                       # no solution, or a segment too short
            continue
        a = F(-F(c + F(np.sqrt(sigma))))
        if F(0.0) <= a and a <= F(max_fraction * rr):        # the entry point lies on the segment
            a = F(a / rr)
            max_fraction, best = a, i                        # ReportFixture returns the fraction
    return best, max_fraction


def raycast_f64(centres, radius, p1, p2, active=None):
    """(hit, fraction, margin in fraction, margin in metres) in float64. The margins are the smallest
    distance of any decision from its boundary: entry fractions from 0, from 1 and from the winner's,
    and centre distances from the line and from the origin against r. A circle the line misses by
    more than the lateral margin, or whose entry lies beyond the fraction margin, takes no part."""
    p1 = np.asarray(p1, np.float64)
    d = np.asarray(p2, np.float64) - p1
    L2 = float(d @ d)
    L = np.sqrt(L2)
    r = float(radius)
    ts, lat = [], np.inf
    for i, c in enumerate(np.asarray(centres, np.float64)):
        if active is not None and not active[i]:
            continue
        s = p1 - c
        dist = np.sqrt(float(s @ s))
        perp = abs(float(s[0] * d[1] - s[1] * d[0])) / L
        lat = min(lat, abs(dist - r), abs(perp - r))
        disc = float(s @ d) ** 2 - L2 * (float(s @ s) - r * r)
        if disc < 0.0:
            continue
        t = (-float(s @ d) - np.sqrt(disc)) / L2
        ts.append((t, i, dist > r))
    ok = [(t, i) for t, i, outside in ts if outside and 0.0 <= t <= 1.0]
    hit, frac = (-1, 1.0) if not ok else (min(ok)[1], min(ok)[0])
    mfrac = np.inf
    for t, i, _ in ts:
        mfrac = min(mfrac, abs(t), abs(t - 1.0))
        if i != hit and hit >= 0:
            mfrac = min(mfrac, abs(t - frac))
    return hit, frac, mfrac, lat
