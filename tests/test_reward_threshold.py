"""The binary reward without a square root (gym-macm_amd/csrc/reward_threshold.h): the wave kernels
test td2 < T for the float32 threshold T the host derives from reward_radius once per world, where
the reference tests sqrt(float64(td2)) < reward_radius (mvmnt.py:160-179), td2 being the float32
squared distance to the target.

The bar is equality of the two tests for every float32 td2, not closeness: T must be the smallest
float32 whose float64 square root reaches the radius. The host function is built from the library's
own header into a stand-alone program (tools/reward_thr_check.c) and compared with numpy's
correctly rounded float64 sqrt around T, at every binade edge, 0, denormals, +inf and NaN. One GPU
case puts agents at squared distances T, the float32 below and the float32 above, and compares the
rewards of the single step and of the carried rollout with the CPU oracle's."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEFAULT_R = 7.0  # flockSettings._reward_radius / macm_config_default
NAMED_R = [DEFAULT_R, 0.1, 1.0, 35.0, 1e-20, 0.0, -1.0, float("inf"), float("nan")]


@pytest.fixture(scope="module")
def threshold(tmp_path_factory):
    """R (float64 array) -> T (float32 array), by the host's macm_reward_thr2."""
    d = tmp_path_factory.mktemp("reward_thr")
    exe = str(d / "reward_thr_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", os.path.join(REPO, "tools", "reward_thr_check.c"),
                    "-lm", "-o", exe], check=True, cwd=d)

    def fn(R):
        R = np.atleast_1d(np.asarray(R, np.float64))
        text = "".join(f"{b:016x}\n" for b in R.view(np.uint64).tolist())
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
        T = np.array([int(t, 16) for t in out.split()], np.uint32).view(np.float32)
        assert T.shape == R.shape
        return T
    return fn


def probes(T):
    """Every float32 within 4096 ulps of T (clipped to [0, +inf]), every binade edge with its two
    neighbours, 0, the smallest and largest denormals, the largest finite float32, +inf and NaN."""
    edges = (np.arange(1, 255, dtype=np.uint32) << 23)  # 2^-126 .. 2^127
    fixed = np.concatenate([edges - 1, edges, edges + 1,
                            np.array([0, 1, 2, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000, 0x7FC00000], np.uint32)])
    out = [fixed]
    if not np.isnan(T):
        t = int(np.array(T, np.float32).view(np.uint32))  # T >= +0: bit patterns are ordered
        lo, hi = max(t - 4096, 0), min(t + 4096, 0x7F800000)
        out.append(np.arange(lo, hi + 1, dtype=np.uint32))
    return np.concatenate(out).view(np.float32)


def check(R, T):
    x = probes(T)
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(x.astype(np.float64)) < R
        got = x < T
    bad = np.nonzero(ref != got)[0]
    assert bad.size == 0, f"R = {R!r}, T = {T!r}: differs at td2 = {x[bad[:5]]!r}"


@pytest.mark.parametrize("R", NAMED_R, ids=[repr(r) for r in NAMED_R])
def test_named_radii(threshold, R):
    T = threshold(R)[0]
    check(R, T)
    if not R > 0:  # R <= 0 and NaN: no distance passes
        assert T == 0 and not np.signbit(T)
    if R == float("inf"):
        assert T == F(np.inf)


def test_random_radii(threshold):
    """200 radii: half log-uniform over float32's whole range of square roots (2^-80 .. 2^70, both
    ends beyond it), half uniform in the range worlds use."""
    rng = np.random.default_rng(11)
    R = np.concatenate([2.0 ** rng.uniform(-80, 70, 100), rng.uniform(0.01, 100.0, 100)])
    T = threshold(R)
    for r, t in zip(R.tolist(), T):
        check(r, t)


def test_threshold_is_minimal(threshold):
    """T is the smallest float32 whose float64 sqrt reaches R (which the equality above implies; said
    directly here), also where R * R leaves float32's range at either end."""
    R = np.array([DEFAULT_R, 0.1, 35.0, 1e-20, 1e-23, 1e-30, 1.8e19, 1.9e19, 1e200])
    T = threshold(R)
    for r, t in zip(R.tolist(), T):
        assert np.sqrt(np.float64(t)) >= r
        assert t > 0 and np.sqrt(np.float64(np.nextafter(t, F(-np.inf)))) < r
    assert T[-1] == F(np.inf) and T[-2] == F(np.inf) and np.isfinite(T[-3])
    assert T[5] == np.nextafter(F(0), F(1))


def split_squares(X, rng):
    """float32 (dx, dy) with fl(fl(dx * dx) + fl(dy * dy)) == X exactly (the kernel's and Box2D's
    b2DistanceSquared of a target at the origin and an agent at (-dx, -dy))."""
    X = F(X)
    dx = (rng.uniform(0.2, 0.9, 4000) * np.sqrt(np.float64(X))).astype(np.float32)
    dy0 = np.sqrt(np.float64(X) - dx.astype(np.float64) ** 2).astype(np.float32)
    for k in range(-8, 9):
        dy = (dy0.view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)
        td2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
        hit = np.nonzero(td2 == X)[0]
        if hit.size:
            return dx[hit[0]], dy[hit[0]]
    raise AssertionError(f"no float32 pair with squared length {X!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [DEFAULT_R, 0.1, 35.0])
def test_gpu_rewards_at_the_threshold(threshold, radius):
    """Agent 0 of env 3 d + j sits at squared distance (T-, T, T+)[j] from its target, d = 0, 1 two
    ways to split it into dx and dy; the other agents are parked far from the target and from each
    other. Idle actions and zero velocities: nobody moves, so the step's td2 is the constructed one.
    Rewards of one step() (env_step_w64) and of a 2-step rollout (the carried rollout kernel)
    against the oracle's, and the probes against what they were built to give."""
    import torch
    import constructed as cs
    from test_gpu_parity import make_pair

    T = threshold(radius)[0]
    X = [np.nextafter(T, F(-np.inf)), T, np.nextafter(T, F(np.inf))]
    E, N = 6, 64
    rng = np.random.default_rng(5)
    pos = np.zeros((E, N, 2), np.float32)
    pos[:, :, 0] = 200.0 + 3.0 * np.arange(N)  # parked: a row 3 m apart, 200 m from the target
    pos[:, :, 1] = 200.0
    want = np.zeros((E, N), np.float32)
    for e in range(E):
        dx, dy = split_squares(X[e % 3], rng)
        pos[e, 0] = (-dx, -dy)
        want[e, 0] = 1.0 if e % 3 == 0 else 0.0
    kw = {} if radius == DEFAULT_R else {"_reward_radius": radius}
    vec, orc = make_pair(E, [N], 3, start_spread=400, **kw)
    assert vec.settings.reward_radius == radius
    cs.inject(vec, orc, pos)
    for w in (vec, orc):  # the target at the origin: target - position is (dx, dy) exactly
        st = w.get_state(vec.world.C) if w is orc else w.get_state()
        st["targets"][:] = 0.0
        w.set_state(st)
    idle = np.ones((E, N, 3), np.uint8)
    acts = torch.from_numpy(np.stack([idle, idle])).cuda()
    r = orc.step(idle)
    np.testing.assert_array_equal(r["reward"].astype(np.float32), want)  # the probes probe
    assert not r["collided"].any()
    vec.step(acts[0])
    np.testing.assert_array_equal(vec.world.reward.cpu().numpy(), want)
    np.testing.assert_array_equal(vec.get_state()["pos"], pos)  # nobody moved
    traj = vec.rollout(acts, trajectory=True)
    rew = vec.world.reward if not isinstance(traj, dict) else traj["reward"]
    got = rew.cpu().numpy().reshape(-1, E, N)
    for k in range(got.shape[0]):
        np.testing.assert_array_equal(got[k], want, err_msg=f"rollout step {k}")
    assert vec.status() == 0
