"""macm_world_reset / macm_tdm_reset and the reset_envs calls on the device against CPython's own
``random`` (tests/pyrandom_ref.py), not against the oracle: the host generator that seeds every env
(csrc/py_mt19937.hpp: a one-word key below 2**32, a two-word key from there) and the device generator
that continues each env's stream (csrc/env_reset.hip: the draw kernel, its twists, its chunks of draws
on the big path) are otherwise compared only with oracle/pyrandom.c, the same restatement. Seeds from
2**32 were never run: every other test seeds below 2**31."""
import numpy as np
import pytest
import torch

import pyrandom_ref as ref

pytestmark = pytest.mark.gpu

from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

E = 3  # with SEED_PAIRS: the key's word count changes inside the batch; (2**64 - 4) + 2 is still below 2**64


@pytest.mark.parametrize("seed,env_offset", ref.SEED_PAIRS)
def test_flock_reset_state_is_cpythons(seed, env_offset):
    """The two-word branch of PyMT19937's constructor (key[1] != 0) and uint64 seed + env_offset + e:
    pos, angle and targets after the constructor's reset, before any step, are random.Random's."""
    N, T = 20, 2
    vec = FlockVec(E, n_agents=[N], targets=[i % T for i in range(N)], seed=seed, env_offset=env_offset,
                   device="cuda:0")
    pos, ang, tg = ref.flock_reset(ref.streams(E, seed, env_offset), vec.world.cfg)
    s = vec.get_state()
    np.testing.assert_array_equal(s["targets"], tg)
    np.testing.assert_array_equal(s["pos"], pos)
    np.testing.assert_array_equal(s["angle"], ang)
    assert (s["step_count"] == 0).all() and vec.status() == 0


@pytest.mark.parametrize("seed,env_offset", ref.SEED_PAIRS)
def test_tdm_reset_state_is_cpythons(seed, env_offset):
    """macm_tdm_reset's seeding (the same constructor, combat.py's draw order) at one- and two-word keys."""
    w = TdmWorld(tdm_config([3, 2, 2]), E, device="cuda:0")
    w.reset(seed, env_offset)
    pos, ang = ref.tdm_reset(ref.streams(E, seed, env_offset), w.cfg)
    s = w.get_state()
    np.testing.assert_array_equal(s["pos"], pos)
    np.testing.assert_array_equal(s["angle"], ang)
    assert (s["health"] == w.cfg.init_health).all() and w.status() == 0


@pytest.mark.parametrize("N,spread", [(64, 20.0), (1025, 30.0)])
def test_flock_reset_envs_continue_cpythons_streams(N, spread):
    """Five reset_envs with a mask: the device draw kernel (env_reset.hip) continues each masked env's
    stream as CPython does, across twists of the 624-word state, on the wave path (N = 64: a twist every
    ~1.6 resets) and on the big path's chunks of draws (N = 1025: ~10 twists per reset, a partial last
    chunk); the envs that are not reset keep their poses and their streams (the last reset of all envs
    would show a stream that had advanced). Seeded so that env 0 has a one-word and envs 1, 2 a two-word
    key."""
    seed = (1 << 32) - 1
    vec = FlockVec(E, n_agents=[N], seed=seed, device="cuda:0", start_spread=spread)
    cfg = vec.world.cfg
    rs = ref.streams(E, seed, 0)
    pos, ang, tg = ref.flock_reset(rs, cfg)
    masks = [[1, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 0, 1], [1, 1, 1]]  # env 1: only in the last
    for rnd, m in enumerate(masks):
        vec.reset_envs(torch.tensor(m, dtype=torch.uint8, device="cuda:0"))
        ref.redraw(rs, cfg, m, pos, ang, ref.flock_agents)
        s = vec.get_state()
        np.testing.assert_array_equal(s["pos"], pos, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["angle"], ang, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["targets"], tg, err_msg=f"reset {rnd}: targets are kept")
    assert vec.status() == 0


def test_tdm_reset_envs_continue_cpythons_streams():
    """macm_tdm_reset_envs' draws (env_reset.hip in TDM mode: x scaled by team + width / 2) on the
    workgroup path, [33, 32]: 195 draws per reset, a twist every ~1.6 resets."""
    seed = (1 << 32) - 1
    w = TdmWorld(tdm_config([33, 32]), E, device="cuda:0")
    w.reset(seed, 0)
    rs = ref.streams(E, seed, 0)
    pos, ang = ref.tdm_reset(rs, w.cfg)
    for rnd, m in enumerate([[0, 1, 1], [0, 1, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 1, 1]]):
        w.reset_envs(torch.tensor(m, dtype=torch.uint8, device="cuda:0"))
        ref.redraw(rs, w.cfg, m, pos, ang, ref.tdm_agents)
        s = w.get_state()
        np.testing.assert_array_equal(s["pos"], pos, err_msg=f"reset {rnd}")
        np.testing.assert_array_equal(s["angle"], ang, err_msg=f"reset {rnd}")
    assert w.status() == 0


def test_flockvec_refuses_a_negative_seed():
    """FlockVec(seed=-1) is not the env its docstring names (CPython would seed abs(-1)): ValueError,
    through World.reset's range check (tests/test_host_seed_range.py has the cases)."""
    with pytest.raises(ValueError):
        FlockVec(2, n_agents=[4], seed=-1, device="cuda:0")
    with pytest.raises(ValueError):
        FlockVec(2, n_agents=[4], seed=(1 << 64) - 1, device="cuda:0")  # env 1's seed would be 2**64
