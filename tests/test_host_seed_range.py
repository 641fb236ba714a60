"""World.reset / TdmWorld.reset (and so FlockVec) refuse seeds whose documented meaning, env e after
``random.seed(seed + env_offset + e)``, the C-ABI cannot honour: it takes seed as uint64_t and
env_offset as int64_t, where ctypes would wrap a negative or too-large int modulo 2**64 without a
word, while CPython seeds abs(seed) or a longer key. The check is a host function (no GPU needed);
the handles are built without a device world, so that reset() reaches only the check."""
import pytest

from gym_macm.tdm_world import TdmWorld
from gym_macm.world import World, check_seed_range

BAD = [
    (-1, 0, 1),                      # CPython: abs(seed)
    (-5, 10, 4),                     # negative seed, even where every env's sum is positive
    (3, -4, 2),                      # env 0's seed is -1
    (0, -1, 1),
    ((1 << 64) - 2, 0, 3),           # the last env's seed is 2**64: a three-word key
    (1 << 64, 0, 1),
    ((1 << 63), (1 << 63) - 1, 2),   # reached through env_offset
    (1 << 64, -(1 << 63), 1),        # seed itself does not fit uint64_t
    (0, 1 << 63, 1),                 # env_offset does not fit int64_t
]
GOOD = [
    (0, 0, 1), ((1 << 32) - 2, 0, 4), ((1 << 64) - 4, 0, 4), (5, (1 << 32) - 3, 3), ((1 << 63) - 3, 1, 3),
    (7, -7, 2),                      # env 0's seed is 0
    ((1 << 64) - 1, -(1 << 63), 4),
]


@pytest.mark.parametrize("seed,env_offset,E", BAD)
def test_seeds_outside_the_abi_range_raise(seed, env_offset, E):
    with pytest.raises(ValueError):
        check_seed_range(seed, env_offset, E)


@pytest.mark.parametrize("seed,env_offset,E", GOOD)
def test_seeds_inside_the_abi_range_pass(seed, env_offset, E):
    assert check_seed_range(seed, env_offset, E) == (seed, env_offset)


@pytest.mark.parametrize("cls", [World, TdmWorld])
def test_reset_checks_before_it_calls_the_library(cls):
    """reset() of a handle without a library or device world behind it: the refusal comes first (a
    reset that reached the C-ABI would fail on the missing attributes instead)."""
    w = cls.__new__(cls)
    w.E = 3
    for seed, off in ((-1, 0), ((1 << 64) - 2, 0), (2, -3)):
        with pytest.raises(ValueError):
            w.reset(seed, off)
    w.__dict__.clear()  # __del__ finds no handle
