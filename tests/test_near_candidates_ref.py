"""The candidate-list rule of the Flock rollout kernels' nearest neighbour (tests/near_candidates_ref.py,
csrc/flock_step_w64.hip above near_build), without a GPU: over oracle position traces and constructed
cases the list's nearest is the plain float32 sweep's for every agent-step, index and value, and at
the default spread the rule really takes list steps (a rule that always fell back would pass the
first condition alone)."""
import numpy as np
import pytest

import near_candidates_ref as R

E, N, K = 32, 64, 300


@pytest.fixture(scope="module")
def traces():
    return {"default": R.oracle_trace(E, N, K, seed=3)[0], "spread6": R.oracle_trace(E, N, K, seed=3, start_spread=6)[0]}


def test_default_spread_trace(traces):
    wrong, kinds, largest = R.run_trace(traces["default"])
    assert wrong == 0
    frac = (kinds == R.LIST).mean()
    print(f"list {frac:.3f} rebuild {(kinds == R.REBUILD).mean():.3f} plain {(kinds == R.PLAIN).mean():.3f} "
          f"largest list mean {largest[kinds == R.LIST].mean():.2f}")
    assert frac >= 0.5, frac


def test_default_spread_trace_as_a_carried_launch(traces):
    """The carried kernel's first step of a launch loads, and a loading step takes the plain sweep."""
    wrong, kinds, _ = R.run_trace(traces["default"][:100], first_step_plain=True)
    assert wrong == 0 and (kinds[0] == R.PLAIN).all() and (kinds[1] == R.REBUILD).all()


def test_dense_start_trace(traces):
    wrong, kinds, largest = R.run_trace(traces["spread6"])
    assert wrong == 0
    # the dense start goes through every kind: failed rebuilds, the plain steps after them, list steps
    assert (largest[kinds == R.REBUILD] > R.CAP).any()
    for kind in (R.PLAIN, R.LIST, R.REBUILD):
        assert (kinds == kind).any(), kind


def drift(pos, K, step, seed=0):
    """[K, 1, N, 2]: pos with every agent moving `step` metres per step in a direction of its own."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, size=pos.shape[0])
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return np.stack([pos + d * (step * k) for k in range(K)]).astype(np.float32)[:, None]


def lattice(n, pitch=1.0):
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)[:n]
    return (g * pitch).astype(np.float32)


def assert_trace(trace, kinds_wanted, **kw):
    wrong, kinds, largest = R.run_trace(trace, **kw)
    assert wrong == 0
    for kind in kinds_wanted:
        assert (kinds == kind).any(), (kind, kinds.ravel())
    return kinds, largest


def test_exact_ties_on_a_lattice():
    """Pitch 2 m: four neighbours at exactly the same d2, the lowest index wins; the lattice stays put
    (list steps with every tie inside the list), then one agent walks through it."""
    pos = lattice(64, 2.0)
    rng = np.random.default_rng(1)
    pos = pos[rng.permutation(64)]  # index order unrelated to the geometry
    still = np.repeat(pos[None, None], 6, axis=0)
    kinds, largest = assert_trace(still, (R.REBUILD, R.LIST))
    assert largest.max() <= R.CAP
    best, bj = R.plain_nearest(pos)
    d2 = R.d2_matrix(pos)
    assert ((d2 == best[:, None]).sum(axis=1) >= 2).all(), "every agent has tied nearest neighbours"
    assert (bj == (d2 == best[:, None]).argmax(axis=1)).all()
    walk = still.repeat(10, axis=0).copy()
    walk[:, 0, 5, 0] += np.arange(walk.shape[0], dtype=np.float32) * np.float32(0.125)  # exact steps: new ties
    assert_trace(walk, (R.REBUILD, R.LIST))


def test_two_agents_at_the_same_point():
    pos = lattice(64, 2.0)
    pos[40] = pos[7]
    trace = drift(pos, 30, 0.0)
    trace[:, 0, 40] = trace[:, 0, 7]  # d2 = 0 for the pair, at every step
    kinds, _ = assert_trace(trace, (R.REBUILD, R.LIST))
    best, bj = R.plain_nearest(trace[3, 0])
    assert best[7] == 0 and bj[7] == 40 and bj[40] == 7
    moving = drift(pos, 30, 0.02, seed=2)
    moving[:, 0, 40] = moving[:, 0, 7]
    assert_trace(moving, (R.REBUILD, R.LIST))


def test_an_agent_far_away():
    """10^4 m from the rest: its d2 are ~10^8, where one float32 ulp is 8 m^2, and its nearest is
    decided among records that differ by less than the list margin in distance."""
    pos = lattice(64, 1.5)
    pos[13] = (1.0e4, 3.0)
    kinds, largest = assert_trace(drift(pos, 40, 0.02, seed=3), (R.REBUILD, R.LIST))
    far = pos.copy()
    far[:32] += np.float32(1.0e4)  # two groups 10^4 m apart, both at coarse float32 positions
    assert_trace(drift(far, 40, 0.02, seed=4), (R.REBUILD, R.LIST))


def test_an_agent_at_the_translation_clamp():
    """2 m per step (b2_maxTranslation) through a resting lattice: a rebuild every step, no list step."""
    pos = lattice(64, 1.5)
    trace = np.repeat(pos[None, None], 12, axis=0).copy()
    trace[:, 0, 20, 1] += np.arange(12, dtype=np.float32) * np.float32(2.0)
    kinds, _ = assert_trace(trace, (R.REBUILD,))
    assert not (kinds == R.LIST).any()
    slow = np.repeat(pos[None, None], 12, axis=0).copy()  # just under s / 4 in all: list steps, then a rebuild
    slow[:, 0, 20, 1] += np.arange(12, dtype=np.float32) * np.float32(0.06)
    kinds, _ = assert_trace(slow, (R.REBUILD, R.LIST))
    assert kinds[:, 0].tolist() == [R.REBUILD] + [R.LIST] * 4 + [R.REBUILD] + [R.LIST] * 4 + [R.REBUILD, R.LIST]


def test_a_clump_above_the_cap():
    """14 agents within 0.2 m of each other: each has 13 candidates, the env goes dense, takes the
    plain sweep for RETRY steps, tries again, and waits twice as long after the second failure."""
    pos = lattice(64, 3.0)
    rng = np.random.default_rng(5)
    pos[:14] = np.float32(40.0) + rng.uniform(0, 0.14, size=(14, 2)).astype(np.float32)
    kinds, largest = assert_trace(np.repeat(pos[None, None], 3 * R.RETRY + 4, axis=0), (R.REBUILD, R.PLAIN))
    k = kinds[:, 0].tolist()
    assert k == [R.REBUILD] + [R.PLAIN] * R.RETRY + [R.REBUILD] + [R.PLAIN] * (2 * R.RETRY) + [R.REBUILD, R.PLAIN]
    assert largest[0, 0] == 13
    # the clump disperses: the retry succeeds
    trace = np.repeat(pos[None, None], 3 * R.RETRY, axis=0).copy()
    trace[R.RETRY // 2:, 0, :14] = lattice(14, 3.0) + np.float32(100.0)
    assert_trace(trace, (R.REBUILD, R.PLAIN, R.LIST))


@pytest.mark.parametrize("n", [33, 63, 2, 1])
def test_other_agent_counts(n):
    rng = np.random.default_rng(n)
    pos = (rng.uniform(0, 12, size=(n, 2))).astype(np.float32)
    kinds, _ = assert_trace(drift(pos, 40, 0.02, seed=n), (R.REBUILD, R.LIST) if n >= 2 else (R.PLAIN,))
    if n == 1:
        best, bj = R.plain_nearest(pos)
        assert np.isinf(best[0]) and bj[0] == 1  # the reference's start value, never replaced


def test_margins_err_towards_a_larger_list():
    """The constants are the kernel's: a pad above 1 on the threshold, a move limit below (s / 4)^2."""
    assert R.PAD == np.float32(1 + 2.0 ** -18) and R.PAD > 1
    assert R.MOVE2 < np.float32(0.0625) and R.MOVE2 == np.float32(0.0625 * (1 - 2.0 ** -20))
