"""TDM.get_obs (gym_macm/envs/combat.py:206-227) restated in numpy with exact bits (tests/ only).

The fixed-slot observation [E, N, N-1, 4] of a state, slot k of agent i being the other agent
j = k < i ? k : k + 1, in the arithmetic every device writer claims (csrc/tdm_obs.hpp):

    rel = pos[j] - pos[i]                       float32
    d2  = rel.x * rel.x + rel.y * rel.y         float32 (b2DistanceSquared)
    r   = sqrt(d2)                              float32 obs: in float32; float64 obs: of float64(d2)
    t   = wrap(obs_atan2(rel.y, rel.x) - float64(angle[i]))
    p   = wrap(float64(angle[j]) - float64(angle[i]))
    ally = 1.0 or 0.0
    wrap(t) = t - copysign(2 pi, t) where |t| > pi

and every column +0.0 where either agent is dead. obs_atan2 is csrc/macm_math.h built for the host
(tests/probe/math_forms.c, the `forms` fixture of tests/test_math_forms.py); the device build of that
header is pinned to the host build bit for bit by tests/test_gpu_primitives.py.

tests/test_tdm_obs_ref.py holds this restatement to the oracle (0 differing float32 bit patterns);
tests/test_gpu_tdm_obs_bits.py holds every device writer to this restatement on bits."""
import ctypes
import functools

import numpy as np
import pytest

from test_math_forms import forms  # noqa: F401  (fixture: macm_math.h built for the host)

P, S = ctypes.c_void_p, ctypes.c_size_t
COLUMNS = ("r", "t", "p", "ally")


def wrap_pi(t):
    return np.where(np.abs(t) > np.pi, t - np.copysign(2.0 * np.pi, t), t)


def host_atan2(lib, y, x):
    """obs_atan2 of the current header, elementwise on float64 arrays of one shape."""
    y = np.ascontiguousarray(y, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    assert y.shape == x.shape
    out = np.zeros_like(y)
    lib.forms_obs_atan2_n(P(y.ctypes.data), P(x.ctypes.data), P(out.ctypes.data), S(y.size))
    return out


def other_agent(N):
    """j [N, N-1]: the other agent of slot k of agent i."""
    i = np.arange(N)[:, None]
    k = np.arange(N - 1)[None, :]
    return np.where(k < i, k, k + 1)


def obs_from_state(lib, pos, angle, alive, teams):
    """(obs32 [E, N, N-1, 4] float32, obs64 float64, mask [E, N, N-1] uint8) of the state."""
    pos = np.asarray(pos)
    angle = np.asarray(angle)
    assert pos.dtype == np.float32 and angle.dtype == np.float32, (pos.dtype, angle.dtype)
    E, N = angle.shape
    assert pos.shape == (E, N, 2) and np.shape(alive) == (E, N) and sum(teams) == N
    team = np.repeat(np.arange(len(teams)), teams)
    j = other_agent(N)
    rel = pos[:, j] - pos[:, :, None]                   # [E, N, N-1, 2] float32: other - agent
    rx, ry = rel[..., 0], rel[..., 1]
    d2 = rx * rx + ry * ry
    assert rel.dtype == np.float32 and d2.dtype == np.float32
    a64 = angle.astype(np.float64)
    t = wrap_pi(host_atan2(lib, ry.astype(np.float64), rx.astype(np.float64)) - a64[:, :, None])
    p = wrap_pi(a64[:, j] - a64[:, :, None])
    ally = np.broadcast_to((team[j] == team[:, None]).astype(np.float64), p.shape)
    live = np.asarray(alive) != 0
    m = live[:, j] & live[:, :, None]
    o64 = np.stack([np.sqrt(d2.astype(np.float64)), t, p, ally], -1)
    o32 = np.stack([np.sqrt(d2), t.astype(np.float32), p.astype(np.float32), ally.astype(np.float32)], -1)
    o64[~m] = 0.0
    o32[~m] = 0.0
    return o32, o64, m.astype(np.uint8)


@pytest.fixture(scope="module")
def tdm_obs(forms):  # noqa: F811
    """tdm_obs(pos, angle, alive, teams) -> (obs32, obs64, mask), bound to the host build of the header."""
    return functools.partial(obs_from_state, forms)


def as_bits(a):
    """The array's bit patterns: an unsigned integer view of the same width."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_obs_bits(got, want, ctx, mask=None, angle=None):
    """obs [E, N, N-1, 4] of one width, on bit patterns; the message names the first differing entry as
    (env, agent, slot, column) with both patterns and how many differ per column, and, given the
    expected mask [E, N, N-1] and the angles [E, N], what kind of slot it is: a masked slot, an alive
    pair with equal angles, or another alive pair; with the count of differing entries of each kind."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    g, w = as_bits(got), as_bits(want)
    bad = g != w
    if bad.any():
        e, i, k, c = (int(v) for v in np.argwhere(bad)[0])
        j = k if k < i else k + 1
        digits = 2 * got.dtype.itemsize
        per = ", ".join(f"{COLUMNS[q]}: {int(bad[..., q].sum())}" for q in range(4))
        kinds = ""
        if mask is not None and angle is not None:
            angle = np.asarray(angle)
            masked = np.asarray(mask) == 0
            equal = ~masked & (angle[:, other_agent(angle.shape[1])] == angle[:, :, None])
            slot = bad.any(-1)
            kinds = (f"; in masked slots {int((slot & masked).sum())}, in alive pairs with equal angles "
                     f"{int((slot & equal).sum())}, in other alive pairs {int((slot & ~masked & ~equal).sum())}; the first is "
                     + ("a masked slot" if masked[e, i, k] else
                        f"an alive pair with {'equal ' if equal[e, i, k] else ''}angles {angle[e, i]!r} and {angle[e, j]!r}"))
        raise AssertionError(
            f"{ctx}: {int(bad.sum())} of {bad.size} obs bit patterns differ ({per}); first at env {e} agent {i} "
            f"slot {k} (other agent {j}) column {COLUMNS[c]}: got {int(g[e, i, k, c]):#0{digits + 2}x} "
            f"({got[e, i, k, c]!r}), expected {int(w[e, i, k, c]):#0{digits + 2}x} ({want[e, i, k, c]!r}){kinds}")


def assert_same_mask_bytes(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and want.dtype == np.uint8 and got.shape == want.shape, (ctx, got.dtype, got.shape)
    bad = got != want
    if bad.any():
        e, i, k = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{ctx}: {int(bad.sum())} mask bytes differ; first at env {e} agent {i} slot {k}: "
                             f"got {int(got[e, i, k])}, expected {int(want[e, i, k])}")
