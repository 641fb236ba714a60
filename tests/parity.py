"""Helpers comparing the HIP world against the CPU oracle (tests/ only)."""
import numpy as np

from oracle import OracleFlock

STATE_KEYS = ("pos", "vel", "angle", "fat", "sleep", "targets", "step_count", "time_passed")


def assert_state_equal(gs, os_, ctx=""):
    """Bit-exact state equality (numpy ==, so -0.0 == +0.0; see flock_step_w64.hip
    'Exactness notes' for why signed zeros of velocity may differ)."""
    for k in STATE_KEYS:
        np.testing.assert_array_equal(gs[k], os_[k], err_msg=f"{ctx} state[{k}]")
    np.testing.assert_array_equal(gs["contact_count"], os_["contact_count"], err_msg=f"{ctx} contact_count")
    for e in range(gs["contact_count"].shape[0]):
        n = int(gs["contact_count"][e])
        np.testing.assert_array_equal(gs["contact_ab"][e, :n], os_["contact_ab"][e, :n],
                                      err_msg=f"{ctx} env {e} contact order")
        np.testing.assert_array_equal(gs["contact_imp"][e, :n], os_["contact_imp"][e, :n],
                                      err_msg=f"{ctx} env {e} impulses")


# Observation layouts: which columns of the last axis are distances (or flags), angles, cos/sin.
OBS_LAYOUTS = {
    "flock_polar": dict(exact=(0, 2), angle=(1, 3), cs=()),        # (r, t) of the neighbour, of the target
    "flock_cart": dict(exact=(0, 3), angle=(), cs=(1, 2, 4, 5)),   # (r, cos t, sin t) twice
    "tdm": dict(exact=(0, 3), angle=(1, 2), cs=()),                # (r, t, p, is_ally) per slot
}
ANGLE_ATOL = 1e-14  # goldens.obs_close's angle tolerance on the float64 observations


def flock_layout(obs):
    """The layout name of a Flock observation array, from its width (4: polar, 6: cartesian)."""
    return {4: "flock_polar", 6: "flock_cart"}[obs.shape[-1]]


def _f32_ordinal(x):
    """float32 -> int64, monotonic in the value (adjacent floats differ by 1; -0 and +0 coincide)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def f32_obs_mismatch(gpu_obs, oracle_obs64, layout):
    """Count float32 obs entries differing from the oracle's f64 obs rounded to f32; assert that
    each of them is admissible for its column (layout: a key of OBS_LAYOUTS):

    - distance and flag columns: at most 1 float32 ulp, nothing else;
    - angle and cos/sin columns: at most 1 ulp (the double atan2 / cos / sin of the device and of
      glibc round differently in rare cases), or at most 1e-14 absolute: `atan2 - angle` cancels
      towards 0, where a float64 ulp of the operands is many float32 ulps of the difference;
    - angle columns only: a sign flip where both values are within 2 float32 ulps of pi in magnitude,
      the wrap at exactly +-pi (one ulp for each side's rounding)."""
    cols = OBS_LAYOUTS[layout]
    width = len(cols["exact"]) + len(cols["angle"]) + len(cols["cs"])
    assert gpu_obs.dtype == np.float32 and gpu_obs.shape == oracle_obs64.shape and gpu_obs.shape[-1] == width, \
        (layout, gpu_obs.dtype, gpu_obs.shape, oracle_obs64.shape)
    ref = oracle_obs64.astype(np.float32)
    d = gpu_obs != ref
    if not d.any():
        return 0
    kg, kr = _f32_ordinal(gpu_obs), _f32_ordinal(ref)
    ok = np.abs(kg - kr) <= 1
    loose = np.zeros(gpu_obs.shape[-1], bool)
    loose[list(cols["angle"] + cols["cs"])] = True
    with np.errstate(invalid="ignore"):
        ok |= loose & (np.abs(gpu_obs.astype(np.float64) - ref.astype(np.float64)) <= ANGLE_ATOL)
    angle = np.zeros(gpu_obs.shape[-1], bool)
    angle[list(cols["angle"])] = True
    kpi = int(_f32_ordinal(np.float32(np.pi)).reshape(-1)[0])
    ok |= angle & (np.signbit(gpu_obs) != np.signbit(ref)) & (np.abs(np.abs(kg) - kpi) <= 2) & (np.abs(np.abs(kr) - kpi) <= 2)
    bad = d & ~ok
    if bad.any():
        idx = np.argwhere(bad)[:5]
        rows = "; ".join(f"{tuple(int(v) for v in i)}: gpu {float(gpu_obs[tuple(i)])!r} ({int(gpu_obs[tuple(i)].view(np.uint32)):#010x})"
                         f" ref {float(ref[tuple(i)])!r} ({int(ref[tuple(i)].view(np.uint32)):#010x})" for i in idx)
        raise AssertionError(f"{int(bad.sum())} obs entries outside the {layout} tolerance: {rows}")
    return int(d.sum())


def oracle_for(cfg, tidx, E, seed, env_offset=0):
    return OracleFlock(cfg, tidx, E, seed, env_offset)


def combat_bot(obs, mask):
    """The reference's scripted TDM actor (test_scripts/bots.py:3-16), vectorised over
    the fixed-slot obs [E, N, N-1, 4] (r, t, p, is_ally) + mask: attack the closest
    enemy (first minimal r in list order), turning toward it, walking forward when
    it is within pi/5, attacking when r < 3; idle without enemies. Rows of dead
    agents are idle (they are not stepped)."""
    E, N = obs.shape[0], obs.shape[1]
    enemy = mask.astype(bool) & (obs[..., 3] == 0)
    r = np.where(enemy, obs[..., 0], np.inf)
    k = np.argmin(r, axis=-1)  # first index of the minimum == strict '<' scan
    has = enemy.any(axis=-1)
    sel = np.take_along_axis(obs, k[..., None, None].repeat(4, -1), axis=2)[..., 0, :]
    a = np.ones((E, N, 4), np.uint8)
    a[..., 3] = 0
    t = sel[..., 1]
    a[..., 0] = np.where(has, (np.abs(t) < np.pi / 5).astype(np.uint8) + 1, 1)
    a[..., 2] = np.where(has, (np.sign(t) + 1).astype(np.uint8), 1)
    a[..., 3] = np.where(has, (sel[..., 0] < 3).astype(np.uint8), 0)
    return a


def combat_bot_dict(obs):
    """bots.combat (test_scripts/bots.py:3-16) on one agent's reference-format obs
    dict, for driving the drop-in TDM through its `actors` hook."""
    enemies = [a for a in obs["agents"] if a["type"] == 0]
    if not enemies:
        return np.array([1, 1, 1, 0])
    closest = enemies[0]
    for a in enemies:
        if a["position"][0] < closest["position"][0]:
            closest = a
    rotation = np.sign(closest["position"][1]) + 1
    forward = int(np.abs(closest["position"][1]) < (np.pi / 5)) + 1
    attack = int(closest["position"][0] < 3)
    return np.array([forward, 1, rotation, attack])


def flock_bot(obs):
    """bots.flock (test_scripts/bots.py:37-61), vectorised over Flock obs [..., 4|6]:
    idle within r < 1 of the target, else turn toward it (sign(t) + 1) and walk
    forward when |t| < pi/4 (cartesian: sign(sin t) + 1, forward when cos t > cos(pi/4))."""
    od = obs.shape[-1]
    h = od // 2
    r = obs[..., h]
    a = np.ones(obs.shape[:-1] + (3,), np.uint8)
    if od == 6:
        rot = np.sign(obs[..., h + 2]) + 1
        fwd = (obs[..., h + 1] > np.cos(np.pi / 4)).astype(np.uint8) + 1
    else:
        rot = np.sign(obs[..., h + 1]) + 1
        fwd = (np.abs(obs[..., h + 1]) < (np.pi / 4)).astype(np.uint8) + 1
    far = ~(r < 1)
    a[..., 0] = np.where(far, fwd, 1)
    a[..., 2] = np.where(far, rot.astype(np.uint8), 1)
    return a
