"""The rearranged f64 forms of csrc/macm_math.h on the device.

obs_atan2_core writes its division out (macm_div_f32sums: v_rcp_f64 and the Newton and residual fmas
of the compiler's own `/`, without the scaling and fix-up instructions, which its operands never
need); obs_atan2 and macm_sincos_pair were rearranged besides. tests/test_math_forms.py shows on the
host that the new header equals the earlier one (tests/probe/macm_math_parent.h) bit for bit; here

* the written-out division equals the compiler's `/` on the numerators and denominators the core
  forms (tests/probe/f64_forms_probe.hip), and obs_atan2 of zero pairs is the earlier header's;
* whole worlds: every observation a step writes equals, bit for bit, the EARLIER header evaluated
  on the host on the oracle's state (positions, angles and neighbour ids are bit-exact), rounded as
  write_obs_row rounds; state, rewards and neighbour ids as tests/parity.py compares them;
* a constructed world with an agent on its target (atan2(0, 0)), angle updates that land on
  +-float32(pi) (the wrap), and an angle that is an entry of the action trig's exception table;
* a TDM world and a workgroup-path Flock world, which take the same headers, against their oracles.
"""
import ctypes

import numpy as np
import pytest
import torch

import constructed as cs
import test_gpu_tdm as tdm
from parity import assert_state_equal
from test_action_trig import table_angles
from test_gpu_parity import check_rollout, make_pair, rand_actions
from test_gpu_primitives import P, S, _load, assert_same_bits, run
from test_math_forms import forms  # noqa: F401  (fixture: both headers built for the host)

pytestmark = pytest.mark.gpu

from gym_macm._abi import DEBUG_FORCE_SPILL  # noqa: E402

PI32 = np.float32(np.pi)


# ---- the division ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def forms_probe():
    lib = _load("libmacm_forms_probe.so")
    lib.probe_div_forms.argtypes = [P, P, P, P, S]
    lib.probe_div_forms.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def probe():
    lib = _load("libmacm_probe.so")
    lib.probe_obs_atan2.argtypes = [P, P, P, S]
    lib.probe_obs_atan2.restype = ctypes.c_int
    return lib


def core_operands(y, x):
    """The numerator and denominator obs_atan2_core divides, from float32 (y, x), in numpy float64:
    (2 mn) - mx, mn + (2 mx) and the like round once, as the core's fmas do (the doublings are exact)."""
    ax, ay = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    r0 = mn < 0.4375 * mx
    r1 = ~r0 & (mn < 0.6875 * mx)
    num = np.where(r0, mn, np.where(r1, mn + mn, mn) - mx)
    den = np.where(r0, mx, mn + np.where(r1, mx + mx, mx))
    return num, den


def division_pairs():
    rng = np.random.default_rng(21)
    n = 1_000_000
    y = rng.normal(0, 30, n).astype(np.float32)
    x = rng.normal(0, 30, n).astype(np.float32)
    h = n // 2
    y[h:] *= np.exp2(rng.integers(-60, 61, n - h)).astype(np.float32)
    x[h:] *= np.exp2(rng.integers(-60, 61, n - h)).astype(np.float32)
    # the reduction thresholds and mn = mx, +-2 ulp; magnitudes 2^-149 .. 2^127 against each other
    mxs = rng.uniform(0.5, 64.0, 4096).astype(np.float32)
    edge = [np.nextafter((c * mxs.astype(np.float64)).astype(np.float32), np.float32(s * np.inf)) for c in
            (0.4375, 0.5, 0.6875, 1.0) for s in (-1, 1)] + [(c * mxs.astype(np.float64)).astype(np.float32)
                                                             for c in (0.4375, 0.5, 0.6875, 1.0)]
    mags = np.exp2(np.arange(-149, 128, 4, dtype=np.float64)).astype(np.float32)
    a, b = np.meshgrid(mags, mags)
    y = np.concatenate([y, *edge, a.ravel(), np.zeros_like(mags)])
    x = np.concatenate([x, *[mxs] * len(edge), b.ravel(), mags])
    return y, x


def test_written_out_division_equals_the_compilers(forms_probe):
    y, x = division_pairs()
    num, den = core_operands(y, x)
    assert (den > 0).all() and (np.abs(num) <= den).all()
    got, plain = run(forms_probe.probe_div_forms, [num, den], [(num.shape, np.float64)] * 2, num.size)
    assert_same_bits("macm_div_f32sums(num, den) vs num / den", got, plain, num, den)
    assert_same_bits("device num / den vs numpy", plain, num / den, num, den)


def test_zero_denominator_pairs_are_the_earlier_headers(probe, forms):  # noqa: F811
    """den = 0 only for x = y = 0: the division's NaN never leaves obs_atan2 (the four signed-zero pairs),
    and the pairs around them (one operand the smallest denormal) are the earlier header's as well."""
    tiny = np.float32(2.0 ** -149)
    v = np.array([0.0, -0.0, tiny, -tiny], np.float32)
    y, x = [a.ravel().astype(np.float64) for a in np.meshgrid(v, v)]
    want = np.zeros_like(y)
    forms.forms_parent_atan2_n(P(y.ctypes.data), P(x.ctypes.data), P(want.ctypes.data), S(y.size))
    got = run(probe.probe_obs_atan2, [y, x], [(y.shape, np.float64)], y.size)
    assert np.isfinite(got).all()
    assert_same_bits("obs_atan2 around (0, 0)", got, want, y, x)


# ---- whole worlds -----------------------------------------------------------------------------------

def wrap_pi(t):
    return np.where(np.abs(t) > np.pi, t - np.copysign(2.0 * np.pi, t), t)


def expected_obs(forms, st, nbr, tidx):  # noqa: F811
    """Flock.get_obs in the step's arithmetic (write_obs, csrc/flock_step_w64.hip) from a state and the
    neighbour ids, with the EARLIER obs_atan2: ([E, N, 4] float32, [E, N, 4] float64)."""
    pos, ang = st["pos"].astype(np.float32), st["angle"].astype(np.float32)
    E, N = ang.shape
    other = np.take_along_axis(pos, nbr.astype(np.int64)[..., None].repeat(2, -1), axis=1)
    rel = other - pos                                   # float32, other - self
    tg = st["targets"].astype(np.float32)[:, np.asarray(tidx, np.int64)]
    trel = tg - pos
    best = rel[..., 0] * rel[..., 0] + rel[..., 1] * rel[..., 1]
    td2 = trel[..., 0] * trel[..., 0] + trel[..., 1] * trel[..., 1]
    assert best.dtype == np.float32 and td2.dtype == np.float32

    def angle(r):
        y = np.ascontiguousarray(r[..., 1].astype(np.float64).ravel())
        x = np.ascontiguousarray(r[..., 0].astype(np.float64).ravel())
        out = np.zeros_like(y)
        forms.forms_parent_atan2_n(P(y.ctypes.data), P(x.ctypes.data), P(out.ctypes.data), S(y.size))
        return wrap_pi(out.reshape(E, N) - ang.astype(np.float64))

    t0, t1 = angle(rel), angle(trel)
    o64 = np.stack([np.sqrt(best.astype(np.float64)), t0, np.sqrt(td2.astype(np.float64)), t1], axis=-1)
    o32 = np.stack([np.sqrt(best), t0.astype(np.float32), np.sqrt(td2), t1.astype(np.float32)], axis=-1)
    return o32, o64


def same_obs(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    assert not bad.any(), (f"{ctx}: {int(bad.sum())} obs entries differ from the earlier header's, first at "
                           f"{tuple(int(v) for v in np.argwhere(bad)[0])}: {got[bad][0]!r} vs {want[bad][0]!r}")


WORLDS = {"3x64": (3, 64), "3x33": (3, 33), "3x2": (3, 2), "2x32": (2, 32)}
STEPS = 40
_REF = {}


def reference(forms, name):  # noqa: F811
    """The oracle's rollout of a world, once: actions, per-step rewards / neighbour ids / expected
    observations (both widths), and the final state. Shared by the four cases of a world."""
    if name not in _REF:
        E, N = WORLDS[name]
        vec, orc = make_pair(E, [N], seed=77)  # the vec only names the world (targets, capacity)
        rng = np.random.default_rng(5)
        acts = np.stack([rand_actions(rng, E, N) for _ in range(STEPS)])
        rows = []
        for t in range(STEPS):
            r = orc.step(acts[t])
            o32, o64 = expected_obs(forms, orc.get_state(vec.world.C), r["nbr_id"], vec.targets_idx)
            rows.append(dict(reward=r["reward"].astype(np.float32), nbr=r["nbr_id"].copy(), o32=o32, o64=o64))
        _REF[name] = dict(acts=acts, rows=rows, state=orc.get_state(vec.world.C))
        for v in _REF[name]["state"].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[name]


@pytest.mark.parametrize("obs_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["rollout", "steps"])
@pytest.mark.parametrize("name", list(WORLDS))
def test_world_observations_are_the_earlier_headers_bits(forms, name, form, obs_f64):  # noqa: F811
    E, N = WORLDS[name]
    ref = reference(forms, name)
    vec, _ = make_pair(E, [N], seed=77, obs_dtype=torch.float64 if obs_f64 else torch.float32)
    key = "o64" if obs_f64 else "o32"
    acts = torch.from_numpy(ref["acts"]).cuda()
    if form == "rollout":
        traj = vec.rollout(acts, trajectory=True)
        obs, nbr, rew = (traj[k].cpu().numpy() for k in ("obs", "nbr_id", "reward"))
    else:
        outs = [[o.cpu().numpy() for o in vec.step(acts[t])[:3]] for t in range(STEPS)]
        obs, nbr, rew = (np.stack([o[k] for o in outs]) for k in range(3))
    for t, row in enumerate(ref["rows"]):
        np.testing.assert_array_equal(nbr[t], row["nbr"], err_msg=f"nbr step {t}")
        np.testing.assert_array_equal(rew[t], row["reward"], err_msg=f"reward step {t}")
        same_obs(obs[t], row[key], f"{name} {form} step {t}")
    assert_state_equal(vec.get_state(), ref["state"], f"{name} {form} after {STEPS} steps")
    assert vec.status() == 0


# ---- constructed ------------------------------------------------------------------------------------

def landing_angle(target, d):
    """A float32 angle a with float32(a + d) == target (the step's angle update, in float64 then rounded)."""
    a = np.float32(float(target) - d)
    for k in range(-4, 5):
        c = cs.step_f32(a, k)
        if np.float32(float(c) + d) == target:
            return c
    raise AssertionError(f"no float32 angle lands on {target!r} with increment {d!r}")


@pytest.mark.parametrize("form", ["rollout", "steps"])
def test_constructed_zero_target_pi_landings_and_table_angle(forms, form):  # noqa: F811
    E, N = 2, 64
    vec, orc = make_pair(E, [N], seed=3)
    from gym_macm.settings import flockSettings
    s = flockSettings()
    d = (1.0 * float(s.agent_rotation_speed)) * (1.0 / float(s.hz))  # (a2 - 1) * rot * (1 / hz), a2 = 2
    st0 = orc.get_state(vec.world.C)
    tg = st0["targets"].astype(np.float32)[:, np.asarray(vec.targets_idx, np.int64)]  # [E, N, 2]
    pos = np.zeros((E, N, 2), np.float32)
    pos[:, 0] = tg[:, 0]                                   # agent 0 exactly on its target
    for i in range(1, N):                                  # the rest on a line beside it, 4 m apart
        pos[:, i] = tg[:, 0] + np.array([4.0 * i, 7.0], np.float32)
    ang = st0["angle"].astype(np.float32).copy()
    ang[:, 1] = landing_angle(PI32, d)                     # a2 = 2: lands on float32(pi) > pi, wraps
    ang[:, 2] = -landing_angle(PI32, d)                    # a2 = 0: lands on -float32(pi)
    near = np.float32(table_angles()[0])                   # a table entry (|a| < 4), kept by a2 = 1
    assert abs(float(near)) < 4.0
    ang[:, 3] = near
    ang[:, 4] = -near
    cs.inject(vec, orc, pos, angle=ang)
    act = np.ones((3, E, N, 3), np.uint8)
    act[0, :, 1, 2] = 2
    act[0, :, 2, 2] = 0
    act[0, :, 3, 0] = 2                                    # forward force along the table angle
    act[0, :, 4, 1] = 0
    act[1:] = np.random.default_rng(9).integers(0, 3, size=(2, E, N, 3))
    tidx = vec.targets_idx
    rows = []
    for t in range(3):
        r = orc.step(act[t])
        st = orc.get_state(vec.world.C)
        rows.append((r, expected_obs(forms, st, r["nbr_id"], tidx)[0], st))
    st = rows[0][2]
    assert (st["pos"][:, 0] == tg[:, 0]).all(), "agent 0 stays on its target: the atan2(0, 0) path"
    assert (np.abs(st["angle"][:, 1:3]) > 3.14).all() and (st["angle"][:, 3] == near).all()
    o = rows[0][1]                                         # target node of agent 0: r = 0, t = atan2(+0, +0) - angle
    assert (o[:, 0, 2] == 0).all() and (o[:, 0, 3] == wrap_pi(-st["angle"][:, 0].astype(np.float64)).astype(np.float32)).all()
    a = torch.from_numpy(act).cuda()
    if form == "rollout":
        traj = vec.rollout(a, trajectory=True)
        obs, nbr, rew = (traj[k].cpu().numpy() for k in ("obs", "nbr_id", "reward"))
    else:
        outs = [[o.cpu().numpy() for o in vec.step(a[t])[:3]] for t in range(3)]
        obs, nbr, rew = (np.stack([o[k] for o in outs]) for k in range(3))
    for t, (r, o32, _) in enumerate(rows):
        np.testing.assert_array_equal(nbr[t], r["nbr_id"], err_msg=f"nbr step {t}")
        np.testing.assert_array_equal(rew[t], r["reward"].astype(np.float32), err_msg=f"reward step {t}")
        same_obs(obs[t], o32, f"constructed {form} step {t}")
    assert_state_equal(vec.get_state(), rows[-1][2], f"constructed {form}")
    assert vec.status() == 0


# ---- the other paths the headers feed ---------------------------------------------------------------

def test_tdm_world_matches_oracle():
    w, orc = tdm.make_pair(2, [2, 2], seed=17, world_width=8.0, world_height=8.0)
    rng = np.random.default_rng(4)
    tdm.check_rollout(w, orc, 20, lambda o, m: tdm.random_actions(rng, 2, 4))


def test_workgroup_flock_world_matches_oracle():
    vec, orc = make_pair(2, [96], seed=19)
    check_rollout(vec, orc, 10, np.random.default_rng(6))


# The workgroup step (flock_step_wg.hip) and the spill step (flock_spill.hpp) carry their own copies of
# write_obs: the polar observation on bits as above. (The cartesian observation calls the device libm's
# cos / sin, which the host cannot restate bit for bit: it stays at its tolerance.)
OTHER_WRITERS = {"2x96-workgroup": (2, 96, 0), "2x33-spill": (2, 33, DEBUG_FORCE_SPILL)}


@pytest.mark.parametrize("obs_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(OTHER_WRITERS))
def test_workgroup_and_spill_observations_are_the_earlier_headers_bits(forms, name, obs_f64):  # noqa: F811
    E, N, debug = OTHER_WRITERS[name]
    vec, orc = make_pair(E, [N], seed=19, obs_dtype=torch.float64 if obs_f64 else torch.float32)
    if debug:
        vec.world.set_debug(debug)
    rng = np.random.default_rng(6)
    for t in range(10):
        a = rand_actions(rng, E, N)
        obs, nbr = (o.cpu().numpy() for o in vec.step(torch.from_numpy(a).cuda())[:2])
        r = orc.step(a)
        np.testing.assert_array_equal(nbr, r["nbr_id"], err_msg=f"{name} nbr step {t}")
        o32, o64 = expected_obs(forms, orc.get_state(vec.world.C), r["nbr_id"], vec.targets_idx)
        same_obs(obs, o64 if obs_f64 else o32, f"{name} step {t}")
    assert_state_equal(vec.get_state(), orc.get_state(vec.world.C), f"{name} after 10 steps")
    assert vec.status() == 0
    if debug:
        assert vec.spilled() > 0, "no env took the spill step"
