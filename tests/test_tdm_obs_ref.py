"""tests/tdm_obs_ref.py, the bit-exact restatement of TDM.get_obs, against the oracle (CPU only).

The device tests (tests/test_gpu_tdm_obs_bits.py) compare every observation writer with the
restatement on bit patterns, so the restatement itself is held here to the oracle's float64
observation (oracle/tdm_oracle.c: glibc atan2) at the strictest bar the two meet:

* the mask is equal;
* obs32 equals the oracle's observation rounded to float32 on bit patterns: 0 differing entries,
  in random crowded worlds with deaths and along every TDM golden's replay;
* obs64 passes tdm_obs_close (the double atan2 of glibc and of csrc/macm_math.h round differently
  in the last place, which float32 rounding hides in these worlds);
* known answers for the cases the zero signs hang on.

The measured figure (0 differing patterns) is the assertion: a restatement that differed from the
oracle anywhere in these worlds would not be a reference for bits."""
import numpy as np
import pytest

import goldens
from constructed import inject_tdm
from oracle import OracleTDM
from tdm_obs_ref import as_bits, tdm_obs, wrap_pi  # noqa: F401  (tdm_obs: fixture)
from test_math_forms import forms  # noqa: F401  (fixture: macm_math.h built for the host)
from test_oracle_tdm_golden import tdm_obs_close

from gym_macm.tdm_world import tdm_config

PI32 = np.float32(np.pi)

WORLDS = {
    "16x[8,8]": ([8, 8], 16, dict(world_width=8.0, world_height=8.0)),
    "4x[16,16]": ([16, 16], 4, dict(world_width=12.0, world_height=12.0)),
    "4x[1,3]": ([1, 3], 4, dict(world_width=5.0, world_height=5.0)),
    "4x[1,1]": ([1, 1], 4, dict(world_width=4.0, world_height=4.0)),
}
STEPS = 80


def assert_equals_oracle(tdm_obs, st, teams, o_obs, o_mask, ctx):  # noqa: F811
    o32, o64, m = tdm_obs(st["pos"], st["angle"], st["alive"], teams)
    np.testing.assert_array_equal(m, o_mask, err_msg=f"{ctx}: mask")
    want = o_obs.astype(np.float32)
    diff = int((as_bits(o32) != as_bits(want)).sum())
    assert diff == 0, f"{ctx}: {diff} of {o32.size} float32 bit patterns differ from the oracle's"
    for e in range(o64.shape[0]):
        assert tdm_obs_close(o64[e], o_obs[e], o_mask[e]), f"{ctx}: float64 obs, env {e}"
    dead = o_mask == 0
    assert not as_bits(o64)[dead].any() and not as_bits(o32)[dead].any(), f"{ctx}: a masked slot is not all-zero bits"
    assert not as_bits(o_obs)[dead].any(), f"{ctx}: the oracle's masked slots are not all-zero bits"


@pytest.mark.parametrize("name", list(WORLDS))
def test_reference_equals_oracle_in_random_worlds(tdm_obs, name):  # noqa: F811
    teams, E, kw = WORLDS[name]
    N = sum(teams)
    orc = OracleTDM(tdm_config(teams, obs_f64=True, **kw), E, 11)
    o_obs, o_mask = orc.observe()
    assert_equals_oracle(tdm_obs, orc.get_state(), teams, o_obs, o_mask, f"{name} reset")
    rng = np.random.default_rng(3)
    for t in range(STEPS):
        a = rng.integers(0, 3, size=(E, N, 4)).astype(np.uint8)
        a[..., 3] = rng.random((E, N)) < 0.5
        r = orc.step(a)
        assert_equals_oracle(tdm_obs, orc.get_state(), teams, r["obs"], r["mask"], f"{name} step {t}")
    if N > 2:
        assert (orc.get_state()["alive"] == 0).any(), "no death: no masked slot was compared"


@pytest.mark.parametrize("name", goldens.tdm_names())
def test_reference_equals_oracle_along_the_goldens(tdm_obs, name):  # noqa: F811
    g = goldens.load(name)
    teams = list(g["meta"]["n_agents"])
    orc = OracleTDM(goldens.tdm_config(g), 1, g["meta"]["seed"])
    o_obs, o_mask = orc.observe()
    assert_equals_oracle(tdm_obs, orc.get_state(), teams, o_obs, o_mask, f"{name} reset")
    for t in range(g["meta"]["steps"]):
        r = orc.step(g["actions"][t][None])
        st = orc.get_state()
        np.testing.assert_array_equal(st["pos"][0], g["pos"][t], err_msg=f"pos step {t}")
        assert_equals_oracle(tdm_obs, st, teams, r["obs"], r["mask"], f"{name} step {t}")
        # and the reference env's own recorded observation, at the goldens' bar
        o64 = tdm_obs(st["pos"], st["angle"], st["alive"], teams)[1]
        assert tdm_obs_close(o64[0], g["obs"][t], g["mask"][t]), f"{name} step {t}: recorded obs"


# ---- known answers ------------------------------------------------------------------------------------

def one_env(tdm_obs, pos, angle, alive=None, teams=None):  # noqa: F811
    pos = np.asarray(pos, np.float32)[None]
    angle = np.asarray(angle, np.float32)[None]
    N = angle.shape[1]
    alive = np.ones((1, N), np.uint8) if alive is None else np.asarray(alive, np.uint8)[None]
    o32, o64, m = tdm_obs(pos, angle, alive, teams or [N - N // 2, N // 2])
    return o32[0], o64[0], m[0]


def test_masked_slot_is_sixteen_zero_bytes(tdm_obs):  # noqa: F811
    o32, o64, m = one_env(tdm_obs, [[0, 0], [1.5, 2.0], [-3.0, 1.0]], [0.7, -2.0, 3.0], alive=[1, 0, 1])
    assert m.tolist() == [[0, 1], [0, 0], [1, 0]]
    for i, k in ((0, 0), (1, 0), (1, 1), (2, 1)):
        assert o32[i, k].tobytes() == bytes(16), (i, k, o32[i, k])
        assert o64[i, k].tobytes() == bytes(32), (i, k, o64[i, k])
    assert o32[0, 1, 0] == np.float32(np.sqrt(np.float32(10.0))) and o32[2, 0, 0] == o32[0, 1, 0]


@pytest.mark.parametrize("a", [0.0, 0.7, -2.5, float(PI32), -float(PI32)])
def test_equal_angles_give_plus_zero_both_ways(tdm_obs, a):  # noqa: F811
    o32, o64, _ = one_env(tdm_obs, [[0, 0], [2.0, 1.0]], [a, a])
    for o in (o32, o64):
        assert as_bits(o)[0, 0, 2] == 0 and as_bits(o)[1, 0, 2] == 0, o[:, 0, 2]


def test_shared_y_gives_zero_and_plus_pi(tdm_obs):  # noqa: F811
    """yj - yi and yi - yj are both +0: atan2(+0, rx) is +0 for rx > 0 and +pi for rx < 0, never -pi (which a
    writer that flipped the signs of one direction's rel for the other, (-ry, -rx), would give)."""
    o32, o64, _ = one_env(tdm_obs, [[1.0, 2.5], [4.0, 2.5]], [0.0, 0.0])
    assert as_bits(o64)[0, 0, 1] == 0, o64[0, 0, 1]
    assert o64[1, 0, 1] == np.pi and as_bits(o32)[1, 0, 1] == as_bits(PI32), o64[1, 0, 1]
    # with angles: t = wrap(atan2 - angle); -angle and pi - angle are exact here, so t + angle restores them
    a = np.array([0.5, -0.25], np.float32)
    o32, o64, _ = one_env(tdm_obs, [[1.0, 2.5], [4.0, 2.5]], a)
    assert o64[0, 0, 1] == -0.5 and o64[0, 0, 1] + 0.5 == 0.0 and not np.signbit(o64[0, 0, 1] + 0.5)
    assert o64[1, 0, 1] == wrap_pi(np.pi + 0.25) and o64[1, 0, 1] < 0  # pi + 0.25 wraps once
    o32, o64, _ = one_env(tdm_obs, [[1.0, 2.5], [4.0, 2.5]], [0.5, 0.25])
    assert o64[1, 0, 1] + 0.25 == np.pi
    # shared x: +-pi/2, each direction its own sign
    o32, o64, _ = one_env(tdm_obs, [[1.0, 2.5], [1.0, 4.5]], [0.0, 0.0])
    assert o64[0, 0, 1] == np.pi / 2 and o64[1, 0, 1] == -np.pi / 2


def test_coincident_agents(tdm_obs):  # noqa: F811
    a = np.array([0.75, -3.0], np.float32)
    o32, o64, m = one_env(tdm_obs, [[1.25, -2.0], [1.25, -2.0]], a)
    assert m.all()
    for o in (o32, o64):
        assert as_bits(o)[0, 0, 0] == 0 and as_bits(o)[1, 0, 0] == 0       # r = +0
    assert o64[0, 0, 1] == -0.75 and o64[1, 0, 1] == 3.0                   # t = wrap(+0 - angle)
    o32, o64, _ = one_env(tdm_obs, [[0, 0], [0, 0]], [float(PI32), -float(PI32)])
    assert o64[0, 0, 1] == -float(PI32) + 2 * np.pi                        # |0 - float32(pi)| > pi wraps
    assert o64[1, 0, 1] == float(PI32) - 2 * np.pi


def test_pi_angles_wrap_p_once(tdm_obs):  # noqa: F811
    assert float(PI32) > np.pi
    o32, o64, _ = one_env(tdm_obs, [[0, 0], [3.0, 1.0]], [float(PI32), -float(PI32)])
    d = -2.0 * float(PI32)                                                # angle_j - angle_i for agent 0, exact
    assert o64[0, 0, 2] == d + 2 * np.pi and o64[1, 0, 2] == -d - 2 * np.pi
    assert abs(o64[0, 0, 2]) < 1e-6 and o64[0, 0, 2] < 0 < o64[1, 0, 2]   # one wrap, not two: close to zero
    assert as_bits(o32)[0, 0, 2] == as_bits(np.float32(d + 2 * np.pi))


def test_injected_states_equal_the_oracle(tdm_obs):  # noqa: F811
    """Constructed states through the oracle's own observation: equal angles, +-float32(pi), shared x and y,
    |rx| == |ry|, a coincident pair and dead agents; float32 bit patterns equal, masked slots zero."""
    teams, E = [3, 3], 2
    orc = OracleTDM(tdm_config(teams, obs_f64=True, world_width=30.0, world_height=30.0), E, 5)
    pos = np.array([[[0, 0], [1.5, 0], [0, 1.5], [1.5, 1.5], [3.0, 0], [3.0, 3.0]],
                    [[0, 0], [0, 0], [2.0, 2.0], [4.0, 0], [4.0, 2.0], [-2.0, 2.0]]], np.float32)
    ang = np.array([[0.7, 0.7, PI32, -PI32, 0.7, -2.5], [PI32, PI32, 0.0, 0.0, -PI32, 1.0]], np.float32)
    alive = np.array([[1, 1, 0, 1, 1, 0], [1, 1, 1, 1, 1, 1]], np.uint8)
    inject_tdm(None, orc, pos, ang, alive=alive, health=alive.astype(np.float64))
    o_obs, o_mask = orc.observe()
    st = orc.get_state()
    assert (st["pos"] == pos).all() and (as_bits(st["angle"]) == as_bits(ang)).all()
    assert_equals_oracle(tdm_obs, st, teams, o_obs, o_mask, "injected")
    assert (o_mask[0] == 0).any() and o_mask[1].all()
