"""The CPU oracle's generator (oracle/pyrandom.c) against CPython's own ``random``. The device
generator (csrc/env_reset.hip) and the host's (csrc/py_mt19937.hpp) are tested against the oracle,
and oracle/pyrandom.c is the same restatement of Modules/_randommodule.c as the host's: an error made
in both would go unseen. These tests pin the oracle to the real generator where the restatement
branches: keys of one and of two 32-bit words (seeds below and from 2**32, the boundary inside one
batch and reached through env_offset alone), the second word's top bit, the last seeds below 2**64,
and the state's twists (624 words: five reset_envs of 3 N draws of two words each cross several at
N = 64 and N = 1025). No GPU."""
import numpy as np
import pytest

import pyrandom_ref as ref
from oracle import OracleFlock, OracleTDM

from gym_macm.settings import flockSettings, to_config
from gym_macm.tdm_world import tdm_config

E = 4  # (2**64 - 4, 0): the four last seeds the ABI can name


@pytest.mark.parametrize("seed,env_offset", ref.SEED_PAIRS)
def test_flock_reset_poses_are_cpythons(seed, env_offset):
    """OracleFlock's reset (pyrandom.c seeded with a one- or two-word key per env) against
    random.Random(seed + env_offset + e) drawn in Flock.__init__'s order, two targets so that the
    target draws come first for both."""
    N, T = 7, 2
    cfg = to_config(flockSettings(), N, T, obs_f64=True)
    orc = OracleFlock(cfg, [i % T for i in range(N)], E, seed, env_offset)
    pos, ang, tg = ref.flock_reset(ref.streams(E, seed, env_offset), cfg)
    s = orc.get_state(N * (N - 1) // 2)
    np.testing.assert_array_equal(s["targets"], tg)
    np.testing.assert_array_equal(s["pos"], pos)
    np.testing.assert_array_equal(s["angle"], ang)


@pytest.mark.parametrize("seed,env_offset", ref.SEED_PAIRS)
def test_tdm_reset_poses_are_cpythons(seed, env_offset):
    """OracleTDM's reset against random.Random drawn in TDM.__init__'s order (team by team)."""
    cfg = tdm_config([3, 2, 2], obs_f64=True)
    orc = OracleTDM(cfg, E, seed, env_offset)
    pos, ang = ref.tdm_reset(ref.streams(E, seed, env_offset), cfg)
    s = orc.get_state()
    np.testing.assert_array_equal(s["pos"], pos)
    np.testing.assert_array_equal(s["angle"], ang)


@pytest.mark.parametrize("N", [2, 64, 1025])
def test_flock_reset_envs_continue_cpythons_stream(N):
    """Five reset_envs in a row of one env: each draws the next 3 N values of the stream CPython
    continues, through the twists of the 624-word state (N = 2: none, the index alone advances;
    N = 64: one every ~1.6 resets; N = 1025: ten per reset). The env beside it is never reset: its
    poses stay and its stream does not advance (a last reset of both shows that)."""
    seed = (1 << 32) - 1  # env 0 a one-word key, env 1 a two-word key
    cfg = to_config(flockSettings(start_spread=max(20.0, N / 12.0)), N, 1, obs_f64=True)
    orc = OracleFlock(cfg, None, 2, seed, 0)
    rs = ref.streams(2, seed, 0)
    pos, ang, tg = ref.flock_reset(rs, cfg)
    C = N * (N - 1) // 2
    for rnd in range(5):
        orc.reset_envs(np.array([1, 0], np.uint8))
        ref.redraw(rs, cfg, [1, 0], pos, ang, ref.flock_agents)
        s = orc.get_state(C)
        np.testing.assert_array_equal(s["pos"], pos, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["angle"], ang, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["targets"], tg, err_msg=f"reset {rnd}: targets are kept")
    orc.reset_envs(None)
    ref.redraw(rs, cfg, [1, 1], pos, ang, ref.flock_agents)
    s = orc.get_state(C)
    np.testing.assert_array_equal(s["pos"], pos, err_msg="reset of both")
    np.testing.assert_array_equal(s["angle"], ang, err_msg="reset of both")


def test_tdm_reset_envs_continue_cpythons_stream():
    cfg = tdm_config([33, 32], obs_f64=True)
    seed = (1 << 32) - 1
    orc = OracleTDM(cfg, 2, seed, 0)
    rs = ref.streams(2, seed, 0)
    pos, ang = ref.tdm_reset(rs, cfg)
    for rnd in range(5):  # 195 draws of two words each: a twist every ~1.6 resets
        orc.reset_envs(np.array([0, 1], np.uint8))
        ref.redraw(rs, cfg, [0, 1], pos, ang, ref.tdm_agents)
        s = orc.get_state()
        np.testing.assert_array_equal(s["pos"], pos, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["angle"], ang, err_msg=f"reset {rnd}")
